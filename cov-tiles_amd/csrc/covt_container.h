// covt_container.h -- the two tile container grammars (Gen C: SURVEY.md Appendix A.1; Gen D:
// CovtParser.decodeLayerMetadata, CovtParser.java:574-652, and the column loop of decodeCovt, :56-85), each
// stated once for every serial walker: the host plan (covt_host.cpp), the device plan's wave and lane
// layouts and its property walk (covt_plan_device.hip), and the stand-alone check of
// tests/container_walk/container_walk_check.cc, which g++ builds under the sanitizers.  Plain C++.
//
// A walker is walk_genc / walk_gend over three parts the caller chooses:
//   window   `len`, `Off` (the cursor type: int32_t for tiles under 2 GiB, else int64_t) and peek8(i), the
//            8 bytes at tile offset i in [0, len), little-endian; bytes past the tile are unspecified.
//            ContainerRd<Window> adds the arithmetic (varints, names, record shapes), masked by len.
//   visitor  kStreams / kProps (compile-time: which records it takes -- the other branch compiles away),
//            operator()(const RawStream&) for the Id / Geometry streams, operator()(const PropRaw&) for the
//            property (sub)columns, layer_begin(extent, n_features) and layer_end(data_start): Gen C data
//            offsets are relative to the layer's data start, known once its metadata is read, so the
//            visitor rebases the layer's records then (Gen D offsets are absolute: data_start 0).
//   table    (Gen C) a column's streams, kept while the column is read: storage only, by execution layout
//            (an LDS table, registers with ballots, a plain array, or reading the metadata again).
//              geometry columns   geo_set(s, GeoSm), geo_rewind(s0), geo_get(r, s) with s ascending
//              property columns   set(r, s, PropSm, hashes), get(s), last_role(ns, roles),
//                                 for_each_lang(ns, f) in order, last_named(r, ns, lang_stream)
// The walkers return the status of the first failing check: a layer's metadata checks in reading order,
// then its data bound; a failed tile's records are to be discarded by the caller.
#ifndef COVT_CONTAINER_H
#define COVT_CONTAINER_H

#include <stdint.h>

#include "covt.h"
#include "covt_walk.h"
#include "covt_props_plan.h"

// compile-time packing of a name literal (bytes [from, from + 8) of its first len bytes)
COVT_HD constexpr uint64_t cstrlen(const char* s) { return *s ? 1 + cstrlen(s + 1) : 0; }
COVT_HD constexpr uint64_t pk(const char* s, uint64_t from, uint64_t len) {
    uint64_t v = 0;
    for (uint64_t i = from; i < from + 8 && i < len; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * (i - from));
    return v;
}

// A Gen C geometry column's stream, as the type-ordered layout needs it (type: StreamType of its name, -1: other)
struct GeoSm {
    int32_t type, enc, nv, bl;
};
COVT_HD constexpr bool geo_stream_type(int type) { return type >= ST_GEOMETRY_TYPES && type <= ST_VERTEX_BUFFER; }

// A Gen C property column's stream.  role: PR_* bits of its name; off: relative to the layer's data.
struct PropSm {
    uint32_t h0, h8;  // the table's own (the wave table's hashes of the name and of its bytes from 8 on)
    int32_t noff, nlen, nv, bl;
    int32_t off;
    uint16_t enc, role;
};
enum { PR_PRESENT = 1, PR_DATA = 2, PR_LENGTH = 4, PR_DICTIONARY = 8, PR_PRESENT_LANG = 16 };
constexpr int kLangPrefix = 8;        // strlen("present_"): a localized sub-column's language follows it
constexpr int kPropMaxStreams = 256;  // numStreams bound of a Gen C column (more: COVT_ERR_BAD_HEADER)

template <class Window>
struct ContainerRd : Window {
    using Off = typename Window::Off;
    using Window::len;
    using Window::peek8;
    COVT_HDI int at(Off i) { return (int)(peek8(i) & 0xff); }
    // low n bytes (n <= 8) of x's 7-bit groups packed (LEB128 payload)
    COVT_HDI static uint64_t leb_pack(uint64_t x, int n) {
        x = (n >= 8 ? x : x & ((1ull << (8 * n)) - 1)) & 0x7f7f7f7f7f7f7f7full;
        x = (x & 0x007f007f007f007full) | ((x & 0x7f007f007f007f00ull) >> 1);
        x = (x & 0x00003fff00003fffull) | ((x & 0x3fff00003fff0000ull) >> 2);
        return (x & 0x000000000fffffffull) | ((x & 0x0fffffff00000000ull) >> 4);
    }
    // LEB128 payload of the low n (<= 4) bytes of x
    COVT_HDI static uint32_t leb_pack4(uint32_t x, int n) {
        x = (n >= 4 ? x : x & ((1u << (8 * n)) - 1)) & 0x7f7f7f7fu;
        x = (x & 0x007f007fu) | ((x & 0x7f007f00u) >> 1);
        return (x & 0x3fffu) | ((x & 0x3fff0000u) >> 2);
    }
    // 64-bit LEB128 (Gen C metadata is written with EncodingUtils.encodeVarints), at most 10 bytes; up to
    // 8 bytes decoded from one word
    COVT_HDI bool uv(Off& o, uint64_t& v) {
        const Off avail = (Off)len - o;
        if (avail <= 0) return false;
        const uint64_t w = peek8(o);
        {  // values of up to 4 bytes (nearly all metadata) in 32-bit arithmetic
            const uint32_t w4 = (uint32_t)w;
            uint32_t stop4 = ~w4 & 0x80808080u;
            if (avail < 4) stop4 &= (1u << (8 * (int)avail)) - 1;
            if (stop4) {
                const int n = (__builtin_ctz(stop4) >> 3) + 1;
                v = leb_pack4(w4, n);
                o += n;
                return true;
            }
        }
        uint64_t stop = ~w & 0x8080808080808080ull;
        if (avail < 8) stop &= (1ull << (8 * (int)avail)) - 1;  // only the tile's bytes
        if (stop) {
            const int n = (__builtin_ctzll(stop) >> 3) + 1;
            v = leb_pack(w, n);
            o += n;
            return true;
        }
        if (avail < 8) return false;  // no terminator before the tile's end
        v = leb_pack(w, 8);           // 9- or 10-byte value
        Off q = o + 8;
        COVT_UNROLL1
        for (int i = 8; i < 10; ++i) {
            if (q >= (Off)len) return false;
            const int b = at(q++);
            v |= (uint64_t)(b & 0x7f) << (7 * i);
            if (!(b & 0x80)) {
                o = q;
                return true;
            }
        }
        return false;
    }
    // Gen C stream record tail (numValues, byteLength varints and the encoding byte) from one 64-bit word
    // when both varints have at most 4 bytes and all of it lies in the tile; false (nothing consumed)
    // otherwise, and the caller reads the fields one by one (same values and statuses)
    COVT_HDI bool rec3(Off& o, uint64_t& nv, uint64_t& bl, int& enc) {
        const Off avail = (Off)len - o;
        if (avail < 3) return false;
        const uint64_t w = peek8(o);
        uint64_t stop = ~w & 0x8080808080808080ull;
        if (avail < 8) stop &= (1ull << (8 * (int)avail)) - 1;
        if (!stop) return false;
        const int e1 = __builtin_ctzll(stop) >> 3;  // numValues' last byte
        if (e1 > 3) return false;
        const uint64_t stop2 = stop & (~0ull << (8 * (e1 + 1)));
        if (!stop2) return false;
        const int e2 = __builtin_ctzll(stop2) >> 3;  // byteLength's last byte
        if (e2 - e1 > 4 || e2 + 1 >= avail || e2 + 1 >= 8) return false;
        nv = leb_pack4((uint32_t)w, e1 + 1);
        bl = leb_pack4((uint32_t)(w >> (8 * (e1 + 1))), e2 - e1);
        enc = (int)((w >> (8 * (e2 + 1))) & 0xff);
        o += e2 + 2;
        return true;
    }
    // DecodingUtils.decodeVarint with its 4-byte cap (DecodingUtils.java:157-186), the Gen D metadata's
    // varint: a byte without bit 7 among the first three ends the value, else the fourth byte does
    COVT_HDI bool j4(Off& o, int32_t& v) {
        const Off avail = (Off)len - o;
        if (avail <= 0) return false;
        const uint32_t w4 = (uint32_t)peek8(o);
        const uint32_t stop = ~w4 & 0x808080u;
        const int n = stop ? (__builtin_ctz(stop) >> 3) + 1 : 4;
        if (n > avail) return false;
        v = (int32_t)leb_pack4(w4, n);
        o += n;
        return true;
    }
    // the first 16 bytes of a name at o (n <= 16) packed little-endian (register compares below)
    COVT_HDI void pack16(Off o, uint64_t n, uint64_t& lo, uint64_t& hi) {
        lo = peek8(o);
        if (n < 8) lo &= (1ull << (8 * n)) - 1;
        hi = 0;
        if (n > 8) {
            hi = peek8(o + 8);
            if (n < 16) hi &= (1ull << (8 * (n - 8))) - 1;
        }
    }
    // name at o (n bytes) == the literal (constants evaluated at compile time: a runtime walk of the
    // literal's bytes would be a memory load per character)
#define COVT_IS(r, o, n, str)                                                                          \
    ([&]() {                                                                                           \
        constexpr uint64_t n_ = cstrlen(str), l_ = pk(str, 0, n_), h_ = pk(str, 8, n_);                \
        static_assert(n_ > 0 && n_ <= 16, "names of 1 to 16 bytes");                                   \
        if ((uint64_t)(n) != n_) return false;                                                         \
        uint64_t lo_, hi_;                                                                             \
        (r).pack16((o), n_, lo_, hi_);                                                                 \
        return lo_ == l_ && hi_ == h_;                                                                 \
    }())
    // Gen C stream name -> StreamType (-1: other)
    COVT_HDI int stream_type(Off o, uint64_t n) {
        if (n < 4 || n > 16) return -1;
        uint64_t lo, hi;
        pack16(o, n, lo, hi);
#define COVT_NAME(str, v)                                                               \
    {                                                                                   \
        constexpr uint64_t n_ = cstrlen(str), l_ = pk(str, 0, n_), h_ = pk(str, 8, n_); \
        if (n == n_ && lo == l_ && hi == h_) return v;                                  \
    }
        COVT_NAME("data", ST_DATA)
        COVT_NAME("length", ST_LENGTH)
        COVT_NAME("present", ST_PRESENT)
        COVT_NAME("dictionary", ST_DICTIONARY)
        COVT_NAME("geometry_types", ST_GEOMETRY_TYPES)
        COVT_NAME("geometry_offsets", ST_GEOMETRY_OFFSETS)
        COVT_NAME("part_offsets", ST_PART_OFFSETS)
        COVT_NAME("ring_offsets", ST_RING_OFFSETS)
        COVT_NAME("vertex_offsets", ST_VERTEX_OFFSETS)
        COVT_NAME("vertex_buffer", ST_VERTEX_BUFFER)
#undef COVT_NAME
        return -1;
    }
    // bytes [a, a + n) == bytes [b, b + n) of the tile (two names)
    COVT_HDI bool same(Off a, Off b, int32_t n) {
        for (int32_t i = 0; i < n; i += 8) {
            const int32_t k = n - i < 8 ? n - i : 8;
            const uint64_t m = k >= 8 ? ~0ull : ((1ull << (8 * k)) - 1);
            if ((peek8(a + i) & m) != (peek8(b + i) & m)) return false;
        }
        return true;
    }
    // bytes of an ORC byte-RLE stream of n values at o (control bytes walked, values skipped; -1: it runs
    // past the tile)
    COVT_HDI int32_t byte_rle_length(Off o, int32_t n) {
        Off q = o;
        int64_t done = 0;
        while (done < n) {
            if (q >= (Off)len) return -1;
            const int c = at(q++);
            if (c < 0x80) done += c + 3, q += 1;
            else done += 0x100 - c, q += 0x100 - c;
            if (q > (Off)len) return -1;
        }
        return (int32_t)(q - o);
    }
};

// ---- Gen C ----------------------------------------------------------------------------------------------

// One stream record at o: name, numValues, byteLength, encoding (g.type: the name's StreamType when
// `typed`, read while the window holds the name).  kAgain: a record that passed these checks before, read
// again field by field.
template <bool kAgain = false, class R>
COVT_HDI int genc_stream(R& r, typename R::Off& o, bool typed, typename R::Off& name, uint64_t& sn, GeoSm& g) {
    using Off = typename R::Off;
    const Off len = (Off)r.len;
    uint64_t nv = 0, bl = 0;
    if ((!r.uv(o, sn) || sn > (uint64_t)(len - o)) && !kAgain) return COVT_ERR_TRUNCATED;
    name = o;
    g.type = typed ? r.stream_type(o, sn) : -1;
    o += (Off)sn;
    int enc;
    if (kAgain || !r.rec3(o, nv, bl, enc)) {
        if ((!r.uv(o, nv) || !r.uv(o, bl) || o >= len) && !kAgain) return COVT_ERR_TRUNCATED;
        enc = r.at(o++);
    }
    if ((nv > 0x7fffffff || bl > 0x7fffffff) && !kAgain) return COVT_ERR_BAD_HEADER;
    g.enc = enc;
    g.nv = (int32_t)nv;
    g.bl = (int32_t)bl;
    return COVT_OK;
}

// The localized sub-columns of a string column (LOCALIZED_DICTIONARY: (present_<lang>, <lang>)*, then the
// shared length + dictionary) from its stream table: one per present_<lang> stream, in order, with the last
// stream named <lang> as data and the last length / dictionary
template <class R, class V, class T>
COVT_HDI void prop_localized(R& r, V& v, const T& tab, uint32_t ns, const PropRaw& p) {
    const int32_t ls = tab.last_role(ns, PR_LENGTH), ds = tab.last_role(ns, PR_DICTIONARY);
    const PropSm lsm = tab.get(ls >= 0 ? (uint32_t)ls : 0u), dsm = tab.get(ds >= 0 ? (uint32_t)ds : 0u);
    int32_t lang = 0;
    tab.for_each_lang(ns, [&](uint32_t q) {
        const PropSm sm = tab.get(q);
        const int32_t dd = tab.last_named(r, ns, sm);
        PropRaw x = p;
        x.lang = lang++;
        x.lang_off = sm.noff + kLangPrefix;
        x.lang_len = sm.nlen - kLangPrefix;
        prop_stream(x, 0, sm.off, sm.nv, sm.bl, sm.enc);
        if (dd >= 0) {
            const PropSm dm = tab.get((uint32_t)dd);
            prop_stream(x, 1, dm.off, dm.nv, dm.bl, dm.enc);
        }
        if (ls >= 0) prop_stream(x, 2, lsm.off, lsm.nv, lsm.bl, lsm.enc);
        if (ds >= 0) prop_stream(x, 3, dsm.off, dsm.nv, dsm.bl, dsm.enc);
        v(x);
    });
}

// A tile: version, layer count, then per layer its name, extent, feature and column counts, every column's
// metadata (name, dataType, columnType, stream records) and the columns' data in the same order.  An Id
// column's `data` stream and a geometry column's streams of types 4..9 are the stream records; a geometry
// column's data is laid out in StreamType order (metadata order within a type), then its other streams; every
// other column's in metadata order.  A property column is one record with its streams' roles by name.
template <class R, class V, class T>
COVT_HDI int walk_genc(R& r, V& v, T& tab) {
    using Off = typename R::Off;
    const Off len = (Off)r.len;
    Off o = 0;
    uint64_t version, nlayers;
    if (!r.uv(o, version) || !r.uv(o, nlayers)) return COVT_ERR_TRUNCATED;
    if (version != 1) return COVT_ERR_BAD_HEADER;
    for (uint64_t L = 0; L < nlayers; ++L) {
        uint64_t nlen, extent, nfeat, ncols;
        if (!r.uv(o, nlen) || nlen > (uint64_t)(len - o)) return COVT_ERR_TRUNCATED;
        o += (Off)nlen;
        if (!r.uv(o, extent) || !r.uv(o, nfeat) || !r.uv(o, ncols)) return COVT_ERR_TRUNCATED;
        if (ncols > 4096) return COVT_ERR_BAD_HEADER;
        const int nb = nbits_of_extent(extent);
        int64_t d = 0;  // data bytes of the layer's columns so far
        v.layer_begin(extent > 0x7fffffffull ? -1 : (int32_t)extent, (int32_t)nfeat);
        for (uint32_t c = 0; c < (uint32_t)ncols; ++c) {
            uint64_t cn, ns, sn;
            if (!r.uv(o, cn) || cn > (uint64_t)(len - o) || (uint64_t)(len - o) - cn < 2) return COVT_ERR_TRUNCATED;
            const Off name = o;
            o += (Off)cn;
            const int dtype = r.at(o), ctype = r.at(o + 1);
            o += 2;
            if (!r.uv(o, ns)) return COVT_ERR_TRUNCATED;
            if (ns > (uint64_t)kPropMaxStreams) return COVT_ERR_BAD_HEADER;
            const int kind = COVT_IS(r, name, cn, "id") ? 0 : (COVT_IS(r, name, cn, "geometry") || dtype == 6) ? 1 : 2;
            const bool ordered = V::kStreams && kind == 1;  // its data bytes are counted in type order below
            const bool props = V::kProps && kind == 2;
            const bool localized = props && genc_prop_type(dtype) == COVT_PROP_STRING && ctype == 2;
            const Off s0 = o;
            // geometry stream types seen (a table that keeps nothing is not given the types either: every
            // type is tried)
            uint32_t present = T::kKeepsGeo ? 0u : ~0u;
            for (uint32_t s = 0; s < (uint32_t)ns; ++s) {
                Off sname;
                GeoSm g;
                const int st = genc_stream(r, o, V::kStreams && (kind == 0 || (kind == 1 && T::kKeepsGeo)), sname, sn, g);
                if (st) return st;
                if constexpr (V::kStreams) {
                    if (kind == 0 && g.type == ST_DATA)
                        v(RawStream{(int32_t)L, 0, ST_DATA, g.enc, ctype, g.nv, g.bl, nb, d});
                    if (kind == 1) {
                        tab.geo_set(s, g);
                        if (geo_stream_type(g.type)) present |= 1u << g.type;
                    }
                }
                if constexpr (V::kProps) {
                    if (kind == 2) {  // the name's role, while the window holds it
                        uint32_t role = 0;
                        if (COVT_IS(r, sname, sn, "present")) role |= PR_PRESENT;
                        if (COVT_IS(r, sname, sn, "data")) role |= PR_DATA;
                        if (COVT_IS(r, sname, sn, "length")) role |= PR_LENGTH;
                        if (COVT_IS(r, sname, sn, "dictionary")) role |= PR_DICTIONARY;
                        if (localized && sn > (uint64_t)kLangPrefix && r.peek8(sname) == pk("present_", 0, 8))
                            role |= PR_PRESENT_LANG;
                        tab.set(r, s, PropSm{0u, 0u, (int32_t)sname, (int32_t)sn, g.nv, g.bl, (int32_t)d, (uint16_t)g.enc,
                                             (uint16_t)role}, localized);
                    }
                }
                if (!ordered) d += (int64_t)g.bl;
            }
            if constexpr (V::kStreams) {
                if (kind == 1) {
                    // types 4..9 in type order (metadata order within a type), then (want = 10) the rest
                    present |= 1u << (ST_VERTEX_BUFFER + 1);
                    for (int want = ST_GEOMETRY_TYPES; want <= ST_VERTEX_BUFFER + 1; ++want) {
                        if (!(present >> want & 1)) continue;
                        tab.geo_rewind(s0);
                        for (uint32_t s = 0; s < (uint32_t)ns; ++s) {
                            const GeoSm g = tab.geo_get(r, s);
                            const bool isgeo = geo_stream_type(g.type);
                            if (want <= ST_VERTEX_BUFFER ? g.type != want : isgeo) continue;
                            if (isgeo) v(RawStream{(int32_t)L, 1, g.type, g.enc, ctype, g.nv, g.bl, nb, d});
                            d += (int64_t)g.bl;
                        }
                    }
                }
            }
            if constexpr (V::kProps) {
                if (kind == 2) {
                    PropRaw p = prop_init((int32_t)L, (int32_t)c, (int32_t)nfeat);
                    p.name_off = name;
                    p.name_len = (int32_t)cn;
                    p.type = genc_prop_type(dtype);
                    p.ctype = ctype;
                    if (localized) {
                        prop_localized(r, v, tab, (uint32_t)ns, p);
                    } else {  // in metadata order: the last stream of a role wins
                        for (uint32_t q = 0; q < (uint32_t)ns; ++q) {
                            const PropSm sm = tab.get(q);
                            if (sm.role & PR_PRESENT) prop_stream(p, 0, sm.off, sm.nv, sm.bl, sm.enc);
                            if (sm.role & PR_DATA) prop_stream(p, 1, sm.off, sm.nv, sm.bl, sm.enc);
                            if (sm.role & PR_LENGTH) prop_stream(p, 2, sm.off, sm.nv, sm.bl, sm.enc);
                            if (sm.role & PR_DICTIONARY) prop_stream(p, 3, sm.off, sm.nv, sm.bl, sm.enc);
                        }
                        v(p);
                    }
                }
            }
        }
        // (the data cursor only grows, so this one check fires iff any column's data passes the tile's end)
        if (d > (int64_t)(len - o)) return COVT_ERR_TRUNCATED;
        v.layer_end((int64_t)o);  // the layer's data starts where its metadata ends
        o += (Off)d;
    }
    return o == len ? COVT_OK : COVT_ERR_BAD_HEADER;
}

// The geometry table of a walker that keeps none: geo_get reads the column's metadata again, one stream
// record per call (all of it passed genc_stream's checks on the first reading)
template <class Off>
struct GeoReread {
    static constexpr bool kKeepsGeo = false;
    Off q;
    COVT_HDI void geo_set(uint32_t, const GeoSm&) {}
    COVT_HDI void geo_rewind(Off s0) { q = s0; }
    template <class R>
    COVT_HDI GeoSm geo_get(R& r, uint32_t) {
        Off name;
        uint64_t sn;
        GeoSm g;
        (void)genc_stream<true>(r, q, true, name, sn, g);
        return g;
    }
};

// The table as plain arrays (the host walk)
struct ArrayTab {
    static constexpr bool kKeepsGeo = true;
    GeoSm geo[kPropMaxStreams];
    PropSm ps[kPropMaxStreams];
    void geo_set(uint32_t s, const GeoSm& g) { geo[s] = g; }
    template <class Off>
    void geo_rewind(Off) {}
    template <class R>
    GeoSm geo_get(R&, uint32_t s) const { return geo[s]; }
    template <class R>
    void set(R&, uint32_t s, const PropSm& v, bool) { ps[s] = v; }
    PropSm get(uint32_t s) const { return ps[s]; }
    int32_t last_role(uint32_t ns, uint32_t roles) const {
        for (int32_t s = (int32_t)ns - 1; s >= 0; --s)
            if (ps[s].role & roles) return s;
        return -1;
    }
    template <class F>
    void for_each_lang(uint32_t ns, F&& f) const {
        for (uint32_t s = 0; s < ns; ++s)
            if (ps[s].role & PR_PRESENT_LANG) f(s);
    }
    template <class R>
    int32_t last_named(R& r, uint32_t ns, const PropSm& lang) const {
        const int32_t ll = lang.nlen - kLangPrefix;
        for (int32_t s = (int32_t)ns - 1; s >= 0; --s)
            if (ps[s].nlen == ll && r.same(ps[s].noff, lang.noff + kLangPrefix, ll)) return s;
        return -1;
    }
};

// ---- Gen D ----------------------------------------------------------------------------------------------

// One column's metadata at o: its id (optimized layers, and every layer's first column) or name, the
// dataType / columnType byte and its stream entries (type / encoding byte, numValues, byteLength) up to the
// one that ends the column.  kAgain: a column that passed these checks before, read again for its kind and name.
struct GendColumn {
    int32_t kind, dtype, ctype, name_len;
    int64_t name_off;  // -1: named by id
    uint32_t have;     // stream types present
};
template <bool kAgain, class R>
COVT_HDI int gend_column(R& r, typename R::Off& o, bool by_id, GendColumn& c, typename R::Off& s0) {
    using Off = typename R::Off;
    const Off len = (Off)r.len;
    int32_t x = 0;
    c.name_off = -1;
    c.name_len = 0;
    if (by_id) {
        if (!r.j4(o, x) && !kAgain) return COVT_ERR_TRUNCATED;
        if (kAgain) c.kind = x == 0 ? 0 : (x == 1 ? 1 : 2);
    } else {
        if ((!r.j4(o, x) || x < 0 || x > len - o) && !kAgain) return COVT_ERR_TRUNCATED;
        if (kAgain) {
            c.kind = COVT_IS(r, o, x, "id") ? 0 : COVT_IS(r, o, x, "geometry") ? 1 : 2;
            c.name_off = o;
            c.name_len = x;
        }
        o += x;
    }
    if (!kAgain && o >= len) return COVT_ERR_TRUNCATED;
    const int desc = r.at(o++);
    c.dtype = (desc >> 3) & 0xF;
    c.ctype = desc & 0x7;
    if (!kAgain && c.ctype > 4) return COVT_ERR_BAD_HEADER;
    s0 = o;
    c.have = 0;
    for (;;) {
        if (!kAgain && o >= len) return COVT_ERR_TRUNCATED;
        const int sd = r.at(o++), type = sd >> 4, enc = sd & 0xF;
        if (!kAgain && (type > ST_M || enc > 9)) return COVT_ERR_BAD_HEADER;
        int32_t nv, bl;
        if ((!r.j4(o, nv) || !r.j4(o, bl)) && !kAgain) return COVT_ERR_TRUNCATED;
        c.have |= 1u << type;
        if ((c.dtype == 8 && type == ST_VERTEX_BUFFER) || (type == ST_DATA && c.ctype == CT_PLAIN) ||
            type == ST_DICTIONARY)
            return COVT_OK;
    }
}

// A tile: layers until its end, each a header (bit 0: optimized, i.e. columns named by id), name (named
// layers), extent, feature and column counts, every column's metadata, then the columns' data: a property
// column other than BOOLEAN leads with an implicit present stream (byte-RLE of ceil(features / 8) bytes,
// no metadata: CovtConverter.addNamedColumnMetadata skips PRESENT, :452-458; CovtParser.java:296), and a
// column's streams follow in TreeMap<StreamType> order, the last metadata entry of a type winning.
template <class R, class V>
COVT_HDI int walk_gend(R& r, V& v) {
    using Off = typename R::Off;
    const Off len = (Off)r.len;
    Off o = 0;
    int32_t layer = 0;
    while (o < len) {
        const bool optimized = r.at(o++) & 1;
        int32_t x, extent, nfeat, ncols;
        if (!r.j4(o, x)) return COVT_ERR_TRUNCATED;
        if (!optimized) {  // decodeString: varint length + UTF-8 bytes
            if (x < 0 || x > len - o) return COVT_ERR_TRUNCATED;
            o += x;
        }
        if (!r.j4(o, extent) || !r.j4(o, nfeat) || !r.j4(o, ncols)) return COVT_ERR_TRUNCATED;
        if (ncols < 0 || ncols > 4096) return COVT_ERR_BAD_HEADER;
        GendColumn c;
        Off s0, m = o;
        for (int32_t ci = 0; ci < ncols; ++ci) {  // the metadata's checks, all before the data's
            const int st = gend_column<false>(r, o, optimized || ci == 0, c, s0);
            if (st) return st;
        }
        const int nb = nbits_of_extent((uint32_t)extent);
        int64_t d = o;  // data cursor (64-bit: a column's streams may sum past 2^31 before its bound check)
        v.layer_begin(extent, nfeat);
        for (int32_t ci = 0; ci < ncols; ++ci) {
            (void)gend_column<true>(r, m, optimized || ci == 0, c, s0);
            const int kind = c.kind;
            PropRaw p{};
            if constexpr (V::kProps) p = prop_init(layer, ci, nfeat);
            if (kind == 2 && c.dtype != 0) {
                const int32_t pl = r.byte_rle_length((Off)d, nfeat < 0 ? 0 : (int32_t)(((int64_t)nfeat + 7) / 8));
                if (pl < 0) return COVT_ERR_TRUNCATED;
                if constexpr (V::kProps) prop_stream(p, 0, d, nfeat, pl, 7);
                d += pl;
            }
            for (int type = 0; type <= ST_M; ++type) {
                if (!(c.have >> type & 1) || (kind == 2 && type == ST_PRESENT)) continue;
                int enc = 0;
                int32_t nv = 0, bl = 0;
                for (Off q = s0; q < m;) {  // the last entry of this type
                    const int sd = r.at(q++);
                    int32_t a, b;
                    r.j4(q, a);
                    r.j4(q, b);
                    if ((sd >> 4) == type) enc = sd & 0xF, nv = a, bl = b;
                }
                if constexpr (V::kStreams) {
                    if ((kind == 0 && type == ST_DATA) || (kind == 1 && geo_stream_type(type)))
                        v(RawStream{layer, kind, type, enc, c.ctype, nv, bl, nb, d});
                }
                if (bl < 0) return COVT_ERR_BAD_HEADER;
                if constexpr (V::kProps) {
                    if (type > ST_PRESENT && type <= ST_DICTIONARY) prop_stream(p, type, d, nv, bl, enc);
                }
                d += bl;
            }
            if (d > (int64_t)len) return COVT_ERR_TRUNCATED;
            if constexpr (V::kProps) {
                if (kind == 2) {
                    p.name_off = c.name_off;
                    p.name_len = c.name_len;
                    p.type = gend_prop_type(c.dtype);
                    p.ctype = c.ctype;
                    v(p);
                }
            }
        }
        v.layer_end(0);
        o = (Off)d;
        ++layer;
    }
    return COVT_OK;
}

#endif

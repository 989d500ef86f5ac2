// covt_mvt.hip -- gfx950 MVT geometry encoding of assembled geometry columns (include/covt.h "Geometry as MVT"):
// per feature the command stream of Feature.geometry (zigzag deltas, LEB128 varints) and its GeomType, in the
// column's slice of the mvt buffer.
//
// Seven launches (six without COVT_MVT_ORIENT); no allocation, no atomics, every output element written exactly
// once by one thread (so a captured graph replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the geometry's, then the layout's).
//   2. rings (COVT_MVT_ORIENT only): the segmented reduction of covt_segscan.h under AreaPolicy: the segments are
//      the rings, the value the int64 shoelace S_r over the shifted coordinates (shoelace_term, the measures
//      pass's policy); S_r goes to the upper half of the ring's record.
//   3. features: a thread per feature, the whole wave (a lane per ring, 64 rings a step) for those of kMvNarrow
//      rings or more.  It writes type[f] and walks the feature's rings in order; per ring it fixes k, whether the
//      ring is reversed, and the cursor predecessor: the source index of the last vertex the previous non-empty
//      ring of the feature emits, or -1 for the origin (the wave: a running maximum over the rings).  The record
//      {k, predecessor, flags, the feature's coordinate count} is all the coordinate passes need: an item is
//      local to its coordinate and its ring's record.
//   4. count: the coordinates in chunks of COVT_MVT_CHUNK, a wave per chunk, a row of 128 at a time, in output
//      order: position a + j of the ring [a, b) is item j of the ring, which reads source b - 1 - j if the ring is
//      reversed; the position of a closed polygon ring's last coordinate is no item.  A coordinate's ring as in
//      covt_simplify.hip: the chunk's first by the 64-ary search, then ring starts marked in LDS and a running
//      maximum (DPP).  An item's bytes are the commands in front of it (MoveTo before a ring's first item or a
//      point feature's first, LineTo before a ring's second), its two parameters and ClosePath after a polygon
//      ring's last.  The chunk's byte total goes to chunk_k[chunk].
//   5. scan: per column (a workgroup in small batches, a wave in large ones) the exclusive scan of chunk_k in
//      place -> n_bytes, and n_empty: the features without a coordinate.
//   6. write: pass 4 again; an item's destination is its chunk's base plus its exclusive prefix in the chunk.  The
//      item is put together in registers (at most 16 bytes) and stored with align-1 vector stores of 8, 4, 2 and
//      1 bytes.  The first item of a ring also stores its destination to ring_base[ring].
//   7. offsets: a thread per feature: offsets[f] is the byte prefix at the feature's first coordinate, which (if
//      there is one at or after it) starts a non-empty ring: ring_base of the last ring that starts there; else
//      n_bytes.  So features and rings without items get the right offsets too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt.h"
#include "covt_mvt_plan.h"
#include "covt_segscan.h"

namespace covt {

constexpr int kMvWaves = 4;                // waves per workgroup
constexpr int kMvNarrow = 64;              // rings from which a feature is finished by the whole wave
constexpr int kMvIpl = 4;                  // scan: items per thread and step
constexpr int kMvCoopMaxColumns = 4096;    // scan: batches of at most this many columns get a workgroup per column
constexpr int kMvRows = COVT_MVT_CHUNK / 128;  // count / write: rows of 128 coordinates per chunk
static_assert(COVT_MVT_CHUNK % 128 == 0, "a chunk is whole rows");
static_assert(COVT_MVT_RING_REC == 16, "a ring's record is four words");

// a ring's record: x = k, y = the cursor predecessor (a source index, -1: the origin), z = flags, w = the
// coordinate count of the point feature (kMvFirst); rings kernel: (z, w) = S_r until the features kernel
constexpr uint32_t kMvPoints = 1u;   // a ring of a POINT / MULTIPOINT feature: no commands of its own
constexpr uint32_t kMvFirst = 2u;    // the first non-empty ring of a point feature: MoveTo(w) in front
constexpr uint32_t kMvPolygon = 4u;  // ClosePath after the last item
constexpr uint32_t kMvRev = 8u;      // item j reads source b - 1 - j

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 g_u32x4;
typedef __attribute__((address_space(1))) u32x4 gw_u32x4;
typedef __attribute__((address_space(1))) uint8_t gw_u8;
typedef __attribute__((address_space(1))) uint32_t gw_u32;
typedef __attribute__((address_space(1))) int32_t gw_i32;
typedef __attribute__((address_space(1))) int64_t gw_i64;
typedef __attribute__((address_space(1))) const int64_t g_i64;
typedef uint64_t u64u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint16_t u16u __attribute__((aligned(1)));
typedef __attribute__((address_space(1))) u64u gw_u64u;
typedef __attribute__((address_space(1))) u32u gw_u32u;
typedef __attribute__((address_space(1))) u16u gw_u16u;

// a doubled signed area mod 2^64 under addition
struct AreaV {
    typedef uint64_t T;
    static __device__ __forceinline__ T id() { return 0ull; }
    static __device__ __forceinline__ T join(T a, T b) { return a + b; }
    static __device__ __forceinline__ T sel(bool p, T a, T b) { return p ? a : b; }
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ T dpp(T old, T v) {
        return dpp_move<CTRL, RMASK>(old, v);
    }
    static __device__ __forceinline__ T bcast(T v, int src) { return lane_bcast64(v, src); }
    template <int N>
    struct Lds {
        uint64_t v[N];
        __device__ __forceinline__ T get(int i) const { return v[i]; }
        __device__ __forceinline__ void put(int i, T x) { v[i] = x; }
    };
};

struct MvCol : GeomCol {
    const uint8_t* types;
    uint8_t* o_type;
    int32_t* o_off;
    uint8_t* o_bytes;
    u32x4* rec;                   // the scratch
    uint32_t *ring_base, *chunk_k;
    int64_t byte_cap;
    int32_t s;  // the shift
    bool orient;

    __device__ __forceinline__ int32_t q(int32_t v) const { return v >> s; }
    // coordinate i, clamped into the column (V > 0), shifted
    __device__ __forceinline__ void loadq(int32_t i, int32_t& x, int32_t& y) const {
        load1(clamp0(i, V - 1), x, y);
        x = q(x), y = q(y);
    }
    // chunks of the count and write passes (a column without rings emits nothing)
    __device__ __forceinline__ int32_t chunks() const {
        return R > 0 ? (int32_t)(((int64_t)V + COVT_MVT_CHUNK - 1) / COVT_MVT_CHUNK) : 0;
    }
};
__device__ __forceinline__ MvCol mv_column(const covt_geom_desc& gd, const covt_geom_result& gr, const covt_mvt_desc& md,
                                           const uint8_t* dec, const uint8_t* asmb, uint8_t* out, uint32_t flags,
                                           int32_t shift) {
    MvCol c;
    (GeomCol&)c = geom_col(gd, gr, asmb, md.n_features);
    c.types = dec ? dec + gd.in_off[0] : nullptr;  // (only the features kernel reads types)
    uint8_t* const o = out + md.off;
    c.o_type = o + mvt_type_off(md.n_features);
    c.o_off = (int32_t*)(o + mvt_offsets_off(md.n_features));
    c.o_bytes = o + mvt_bytes_off(md.n_features);
    c.rec = (u32x4*)(o + mvt_ring_rec_off(md.n_features, md.byte_cap));
    c.ring_base = (uint32_t*)(o + mvt_ring_base_off(md.n_features, md.byte_cap, md.ring_cap));
    c.chunk_k = (uint32_t*)(o + mvt_chunk_k_off(md.n_features, md.byte_cap, md.ring_cap));
    c.byte_cap = md.byte_cap;
    c.s = shift;
    c.orient = (flags & COVT_MVT_ORIENT) != 0;
    return c;
}

// The rings of a column as the segments of covt_segscan.h, the value S_r over the shifted coordinates.
struct AreaPolicy {
    typedef AreaV V;
    static constexpr int kWaves = kMvWaves;
    static constexpr int kRows = 1;     // one row of 64 lanes x 2 coordinates per chunk: 128 coordinates
    static constexpr int kWide = 2048;  // coordinates left past a run from which the workgroup finishes a ring
    static constexpr int kIncl = 1;     // an edge's term depends on whether the next coordinate is a head
    static constexpr int kAhead = 1;
    struct Raw {
        i32x4 q;         // shifted
        int32_t tx, ty;  // the coordinate after the chunk, shifted (uniform)
    };

    const MvCol& c;

    __device__ __forceinline__ int32_t count() const { return c.R; }
    __device__ __forceinline__ int32_t items() const { return c.V; }
    __device__ __forceinline__ int32_t first_at(int32_t x) const {
        return seg_first_at(c.R, x, [&](int32_t r) { return c.ring_at(r); });
    }
    __device__ __forceinline__ void open(int32_t) {}
    __device__ __forceinline__ void ensure(int32_t, int32_t) {}
    __device__ __forceinline__ int32_t start(int32_t r) const { return r <= c.R ? c.ring_at(r) : 0x7fffffff; }
    __device__ __forceinline__ void load(Raw& r, int32_t a, int32_t b) const {
        const i32x4 q = c.load2(a + 2 * lane_id(), b);
        r.q = i32x4{c.q(q.x), c.q(q.y), c.q(q.z), c.q(q.w)};
        r.tx = r.ty = 0;
        if (b < c.V) {
            c.load1(b, r.tx, r.ty);
            r.tx = c.q(r.tx), r.ty = c.q(r.ty);
        }
    }
    __device__ __forceinline__ void terms(const Raw& r, int, int32_t a, int32_t p0, int32_t L, int32_t h1, int32_t h2,
                                          uint64_t& t0, uint64_t& t1) const {
        // the coordinate after this lane's two: the next lane's first (lane 63: the one after the chunk)
        const int32_t nx = (int32_t)lane_next((uint32_t)r.q.x, (uint32_t)r.tx);
        const int32_t ny = (int32_t)lane_next((uint32_t)r.q.y, (uint32_t)r.ty);
        const uint64_t e0 = shoelace_term(r.q.x, r.q.y, r.q.z, r.q.w), e1 = shoelace_term(r.q.z, r.q.w, nx, ny);
        t0 = a + p0 + 1 < c.V && h1 == 0 && p0 + 1 < L ? e0 : 0ull;
        t1 = a + p0 + 2 < c.V && h2 == 0 && p0 + 1 < L ? e1 : 0ull;
    }
    // the edges from the coordinates [from, to - 1)
    __device__ __forceinline__ uint64_t tail(int32_t from, int32_t to, int32_t tid, int32_t threads) const {
        uint64_t part = 0;
        for (int32_t i = from + tid; i + 1 < to; i += threads) {
            int32_t x0, y0, x1, y1;
            c.load1(i, x0, y0);
            c.load1(i + 1, x1, y1);
            part += shoelace_term(c.q(x0), c.q(y0), c.q(x1), c.q(y1));
        }
        return part;
    }
    __device__ __forceinline__ void put(int32_t r, uint64_t v, bool) const {
        ((gw_i64*)(c.rec + r))[1] = (int64_t)v;
    }
};

// ---- 1. init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mvt_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                       const covt_geom_result* __restrict__ gres,
                                                       const covt_mvt_desc* __restrict__ mdescs, int64_t n_cols,
                                                       covt_mvt_result* __restrict__ mres) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const covt_mvt_desc md = mdescs[c];
    const covt_geom_desc gd = gdescs[c];
    int32_t st = geom_product_precheck(gd, gres[c], (md.flags & COVT_MVT_TOO_LARGE) != 0, md.off >= 0 && !(md.off & 15),
                                       md.n_features);
    if (st == COVT_OK && (md.ring_cap != gd.ring_cap || md.coord_cap != gd.coord_cap || md.ring_cap < 0 ||
                          md.coord_cap < 0 || md.byte_cap != mvt_capacity(md.n_features, md.ring_cap, md.coord_cap) ||
                          md.byte_cap > INT32_MAX))
        st = COVT_ERR_INVALID_ARG;
    mres[c].status = st;
    if (st != COVT_OK) {  // (an OK column's: the scan's)
        mres[c].n_empty = 0;
        mres[c].n_bytes = 0;
    }
}

// ---- 2. rings -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kMvWaves) void mvt_rings_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, uint32_t flags, int32_t shift, uint8_t* __restrict__ out,
    const covt_mvt_result* __restrict__ mres) {
    __shared__ SegSmem<AreaPolicy> sm;
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, flags, shift);
    AreaPolicy p{c};
    seg_run(p, sm);
}

// ---- 3. features --------------------------------------------------------------------------------------
// what the features pass fixes of a ring but for its predecessor: k, its flags, and the source index of the last
// vertex it emits (-1 if it emits none)
struct MvRing {
    int32_t k;
    uint32_t fl;
    int32_t last;
};
// ring r of a feature of type t (first: it is the first ring of its part)
__device__ __forceinline__ MvRing mv_ring(const MvCol& c, int32_t r, uint32_t t, bool first) {
    const int32_t a = c.ring_at(r), b = c.ring_at(r + 1), m = b - a;
    if (m <= 0) return MvRing{0, 0u, -1};
    if (t == 0u || t == 3u) return MvRing{m, kMvPoints, b - 1};
    if (t != 2u && t != 5u) return MvRing{m, 0u, b - 1};
    int32_t x0, y0, x1, y1;
    c.loadq(a, x0, y0);
    c.loadq(b - 1, x1, y1);
    const bool closed = m >= 2 && x0 == x1 && y0 == y1;
    const int32_t k = m - (closed ? 1 : 0);
    bool rev = false;
    if (c.orient && closed) {
        const int64_t S = ((g_i64*)(c.rec + r))[1];  // (launch 2's)
        rev = first ? S < 0 : S > 0;
    }
    return MvRing{k, kMvPolygon | (rev ? kMvRev : 0u), rev ? a + 1 : a + k - 1};
}
// the record of ring r: pred its cursor predecessor, cnt its feature's coordinate count
__device__ __forceinline__ void mv_put_rec(const MvCol& c, int32_t r, MvRing g, int32_t pred, int32_t cnt) {
    const uint32_t fl = g.fl | (pred < 0 && (g.fl & kMvPoints) && g.k > 0 ? kMvFirst : 0u);
    ((gw_u32x4*)c.rec)[r] = u32x4{(uint32_t)g.k, (uint32_t)pred, fl, (uint32_t)cnt};
}

// blockIdx.x: the column; a thread per feature, its gridDim.y * 64 * kMvWaves threads striding over them
__global__ __launch_bounds__(64 * kMvWaves) void mvt_features_kernel(
    const uint8_t* __restrict__ dec, const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb,
    const covt_geom_result* __restrict__ gres, const covt_mvt_desc* __restrict__ mdescs, uint32_t flags, int32_t shift,
    uint8_t* __restrict__ out, const covt_mvt_result* __restrict__ mres) {
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], dec, asmb, out, flags, shift);
    const int l = lane_id();
    const int32_t threads = (int32_t)(gridDim.y * 64 * kMvWaves);
    // (every lane of a wave runs the same number of steps: the wave finishes its wide features together)
    for (int32_t f0 = (int32_t)(blockIdx.y * 64 * kMvWaves + (threadIdx.x & ~63u)); f0 < c.n; f0 += threads) {
        const int32_t f = f0 + l;
        const bool have = f < c.n;
        int32_t g0 = 0, g1 = 0, r0 = 0, r1 = 0, cnt = 0;
        uint32_t t = 0;
        if (have) {
            g0 = c.geo_at(f), g1 = c.geo_at(f + 1);
            r0 = c.part_at(g0), r1 = c.part_at(g1);
            cnt = max(c.ring_at(r1) - c.ring_at(r0), 0);
            t = (uint32_t)((const g_u8*)c.types)[f];
            ((gw_u8*)c.o_type)[f] = (uint8_t)(t <= 5u ? t % 3u + 1u : 0u);
        }
        // (by rings alone: a feature of many parts but fewer than kMvNarrow rings, that is of many empty parts, is
        // walked part by part by its one thread -- correct and in bounds, only slow for such a column)
        const bool wide = have && r1 - r0 >= kMvNarrow;
        if (have && !wide) {
            int32_t pred = -1;
            for (int32_t g = g0; g < g1; ++g) {
                const int32_t p0 = c.part_at(g), p1 = c.part_at(g + 1);
                for (int32_t r = p0; r < p1; ++r) {
                    const MvRing ring = mv_ring(c, r, t, r == p0);
                    mv_put_rec(c, r, ring, pred, cnt);
                    if (ring.last >= 0) pred = ring.last;
                }
            }
        }
        // the wide features of this step, one after the other by the whole wave, a lane per ring, 64 rings a step
        for (uint64_t m = __ballot(wide); m; m &= m - 1) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const int32_t wg0 = (int32_t)lane_bcast((uint32_t)g0, src), wg1 = (int32_t)lane_bcast((uint32_t)g1, src);
            const int32_t wr0 = (int32_t)lane_bcast((uint32_t)r0, src), wr1 = (int32_t)lane_bcast((uint32_t)r1, src);
            const int32_t wcnt = (int32_t)lane_bcast((uint32_t)cnt, src);
            const uint32_t wt = lane_bcast(t, src);
            const bool need_first = c.orient && (wt == 2u || wt == 5u);
            uint32_t carry = 0;  // the last emitted source index + 1 of the rings before the step (uniform; 0: none)
            for (int32_t rb = wr0; rb < wr1; rb += 64) {
                const int32_t r = rb + l;
                const bool in = r < wr1;
                MvRing ring{0, 0u, -1};
                if (in) {
                    bool first = false;
                    if (need_first) {  // the last part of the feature that starts at or before r: does it start at r
                        int32_t lo = wg0, hi = wg1 - 1;
                        while (lo < hi) {
                            const int32_t mid = lo + (hi - lo + 1) / 2;
                            if (c.part_at(mid) <= r) lo = mid; else hi = mid - 1;
                        }
                        first = c.part_at(lo) == r;
                    }
                    ring = mv_ring(c, r, wt, first);
                }
                const uint32_t inc = incl_max_scan((uint32_t)(ring.last + 1));
                const uint32_t before = max(dpp_move<0x138, 0xf>(0u, inc), carry);
                carry = max(carry, lane_bcast(inc, 63));
                if (in) mv_put_rec(c, r, ring, (int32_t)before - 1, wcnt);
            }
        }
    }
}

// ---- 4. count, 6. write -------------------------------------------------------------------------------
// a uint32 as its varint's bytes, little end first, in a uint64; n: their number
__device__ __forceinline__ uint64_t mv_varint(uint32_t v, int32_t n) {
    const uint64_t x = (uint64_t)v;
    const uint64_t b = (x & 0x7full) | ((x & 0x3f80ull) << 1) | ((x & 0x1fc000ull) << 2) | ((x & 0xfe00000ull) << 3) |
                       ((x & 0xf0000000ull) << 4);
    return b | (0x80808080ull & ((1ull << (8 * (n - 1))) - 1ull));
}

struct MvItem {
    uint64_t lo, hi;  // the item's bytes, little end first
    uint32_t len;
    __device__ __forceinline__ void add(uint64_t bytes, int32_t n) {
        const uint32_t sh = 8u * len;
        if (sh < 64u) {
            lo |= bytes << sh;
            if (sh) hi |= bytes >> (64u - sh);
        } else {
            hi |= bytes << (sh - 64u);
        }
        len += (uint32_t)n;
    }
};

// The item at position i of ring r (valid: i is a coordinate of the chunk): (x, y) the position's own shifted
// coordinate, (bx, by) the one before it.  WRITE: the bytes too.
template <bool WRITE>
__device__ __forceinline__ MvItem mv_item(const MvCol& c, bool valid, int32_t i, int32_t r, int32_t x, int32_t y,
                                          int32_t bx, int32_t by) {
    MvItem it{0ull, 0ull, 0u};
    if (!valid) return it;
    const u32x4 rec = ((g_u32x4*)c.rec)[r];
    const int32_t a = c.ring_at(r), j = i - a, k = (int32_t)rec.x;
    if (j < 0 || j >= k) return it;
    const uint32_t fl = rec.z;
    if (fl & kMvRev) {
        const int32_t src = c.ring_at(r + 1) - 1 - j;
        c.loadq(src, x, y);
        if (j > 0) c.loadq(src + 1, bx, by);
    }
    if (j == 0) {
        bx = by = 0;
        if ((int32_t)rec.y >= 0) c.loadq((int32_t)rec.y, bx, by);
    }
    const uint32_t zx = mvt_zigzag((uint32_t)x - (uint32_t)bx), zy = mvt_zigzag((uint32_t)y - (uint32_t)by);
    // the command in front: MoveTo(count) of a point feature, MoveTo(1), LineTo(k - 1)
    uint32_t cmd = 0;
    if (fl & kMvPoints) {
        if (j == 0 && (fl & kMvFirst)) cmd = (rec.w << 3) | 1u;
    } else if (j == 0) {
        cmd = 9u;
    } else if (j == 1) {
        cmd = ((uint32_t)(k - 1) << 3) | 2u;
    }
    const int32_t nc = cmd ? mvt_varint_len(cmd) : 0, nx = mvt_varint_len(zx), ny = mvt_varint_len(zy);
    const bool close = (fl & kMvPolygon) && j == k - 1;
    if (WRITE) {
        if (cmd) it.add(mv_varint(cmd, nc), nc);
        it.add(mv_varint(zx, nx), nx);
        it.add(mv_varint(zy, ny), ny);
        if (close) it.add(15ull, 1);
    } else {
        it.len = (uint32_t)(nc + nx + ny + (close ? 1 : 0));
    }
    return it;
}

// the item's bytes to bytes[d, d + len) of the column (checked against the capacity): 8, 4, 2, 1 at a time
__device__ __forceinline__ void mv_store(const MvCol& c, uint32_t d, MvItem it) {
    if (!it.len || (int64_t)d + it.len > c.byte_cap) return;
    uint8_t* p = c.o_bytes + d;
    uint64_t v = it.lo;
    if (it.len >= 16u) {
        *(gw_u64u*)p = it.lo;
        *(gw_u64u*)(p + 8) = it.hi;
        return;
    }
    if (it.len & 8u) {
        *(gw_u64u*)p = v;
        v = it.hi, p += 8;
    }
    if (it.len & 4u) {
        *(gw_u32u*)p = (uint32_t)v;
        v >>= 32, p += 4;
    }
    if (it.len & 2u) {
        *(gw_u16u*)p = (uint16_t)v;
        v >>= 16, p += 2;
    }
    if (it.len & 1u) *(gw_u8*)p = (uint8_t)v;
}

// blockIdx.x: the column; a wave per chunk, the column's gridDim.y * kMvWaves waves striding over them.  Per row
// of 128 coordinates the rings that start in it are marked in LDS, a lane per ring (ring + 1 at the start of a
// non-empty ring: one ring per position), and a coordinate's ring is the running maximum of the marks up to it
// (DPP), carried from row to row; the chunk's first by the 64-ary search.
template <bool WRITE>
__global__ __launch_bounds__(64 * kMvWaves) void mvt_stream_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, uint32_t flags, int32_t shift, uint8_t* __restrict__ out,
    const covt_mvt_result* __restrict__ mres) {
    __shared__ __attribute__((aligned(16))) uint32_t marks[kMvWaves][128];
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, flags, shift);
    const int l = lane_id();
    uint32_t* const mark = marks[threadIdx.x >> 6];
    const int32_t chunks = c.chunks();
    const auto ring_at = [&](int32_t r) { return c.ring_at(r); };
    *(uint64_t*)(mark + 2 * l) = 0ull;
    wave_sync();
    for (int32_t ch = uni((int32_t)(blockIdx.y * kMvWaves + (threadIdx.x >> 6))); ch < chunks;
         ch += (int32_t)(gridDim.y * kMvWaves)) {
        const int32_t A = ch * COVT_MVT_CHUNK, B = min(A + COVT_MVT_CHUNK, c.V);
        // the ring of the chunk's first coordinate: the last one that starts at or before it
        const int32_t rlo = clamp0(seg_first_at(c.R, A + 1, ring_at) - 1, c.R - 1);
        uint32_t open = (uint32_t)rlo + 1u;  // ring + 1 of the coordinate before the row (uniform)
        int32_t sc = rlo;                    // the first ring not yet marked (uniform; rlo may start at A itself)
        uint32_t run = WRITE ? (uint32_t)uni((int32_t)((g_u32*)c.chunk_k)[ch]) : 0u;
        int32_t px = 0, py = 0;  // the coordinate before the row, shifted (uniform)
        if (A > 0) c.loadq(A - 1, px, py);
        for (int k = 0; k < kMvRows; ++k) {
            const int32_t a = A + 128 * k, b = min(a + 128, B), i0 = a + 2 * l;
            if (a >= B) break;  // (uniform)
            const i32x4 q = c.load2(i0, B);
            // the rings from sc on that start below b, 64 a step
            for (;;) {
                const int32_t s = sc + l;
                const int32_t st = s < c.R ? c.ring_at(s) : 0x7fffffff;
                const bool in = st < b;  // (a prefix of the lanes)
                if (in && st >= a && c.ring_at(s + 1) > st) mark[st - a] = (uint32_t)s + 1u;
                const int cnt = __popcll(__ballot(in));
                sc += cnt;
                if (cnt < 64) break;
            }
            wave_sync();
            const uint64_t mm = *(const uint64_t*)(mark + 2 * l);
            *(uint64_t*)(mark + 2 * l) = 0ull;  // (the next row's marks follow the wave_sync below)
            const uint32_t m0 = (uint32_t)mm, m1 = (uint32_t)(mm >> 32);
            const uint32_t inc = incl_max_scan(max(m0, m1));
            // the maximum over the lanes before (wave_shr:1), the rows before (open) and the lane's own marks
            const uint32_t r0 = max(max(dpp_move<0x138, 0xf>(0u, inc), open), m0), r1 = max(r0, m1);
            open = max(open, lane_bcast(inc, 63));
            const int32_t x0 = c.q(q.x), y0 = c.q(q.y), x1 = c.q(q.z), y1 = c.q(q.w);
            // the coordinate before this lane's two: the lane before's second (lane 0: the one before the row)
            const int32_t bx = (int32_t)dpp_move<0x138, 0xf>((uint32_t)px, (uint32_t)x1);
            const int32_t by = (int32_t)dpp_move<0x138, 0xf>((uint32_t)py, (uint32_t)y1);
            px = (int32_t)lane_bcast((uint32_t)x1, 63), py = (int32_t)lane_bcast((uint32_t)y1, 63);
            // (r0, r1 are in 1 .. R: open is, and so is every mark)
            const MvItem it0 = mv_item<WRITE>(c, i0 < B, i0, (int32_t)r0 - 1, x0, y0, bx, by);
            const MvItem it1 = mv_item<WRITE>(c, i0 + 1 < B, i0 + 1, (int32_t)r1 - 1, x1, y1, x0, y0);
            const uint32_t own = it0.len + it1.len;
            const uint32_t incl = incl_scan(own);
            if (WRITE) {
                const uint32_t d0 = run + incl - own, d1 = d0 + it0.len;
                mv_store(c, d0, it0);
                mv_store(c, d1, it1);
                // a ring's first position: the byte offset of the ring (offsets kernel)
                if (m0 != 0u && i0 < B) ((gw_u32*)c.ring_base)[m0 - 1u] = d0;
                if (m1 != 0u && i0 + 1 < B) ((gw_u32*)c.ring_base)[m1 - 1u] = d1;
            }
            run += lane_bcast(incl, 63);
            wave_sync();
        }
        if (!WRITE && l == 0) ((gw_u32*)c.chunk_k)[ch] = run;
    }
}

// ---- 5. scan ------------------------------------------------------------------------------------------
// chunk_k -> its exclusive scan in place and n_bytes; n_empty
template <int NW>
__device__ void mvt_scan_column(const MvCol& c, covt_mvt_result* res, AsmSmemT<NW, kMvIpl>& sm) {
    constexpr int K = Coop<NW, kMvIpl>::K;
    const int l = Coop<NW, kMvIpl>::tid();
    auto ioff = [&](int k) { return NW == 1 ? 64 * k + l : kMvIpl * l + k; };
    int buf = 0;
    const int32_t chunks = c.chunks();
    uint32_t base = 0;
    for (int32_t h0 = 0; h0 < chunks; h0 += K) {
        uint32_t x[kMvIpl], ex[kMvIpl], tot;
#pragma unroll
        for (int k = 0; k < kMvIpl; ++k) {
            const int32_t h = h0 + ioff(k);
            x[k] = h < chunks ? ((g_u32*)c.chunk_k)[h] : 0u;
        }
        excl_scan4(sm, buf, x, ex, tot);
#pragma unroll
        for (int k = 0; k < kMvIpl; ++k) {
            const int32_t h = h0 + ioff(k);
            if (h < chunks) ((gw_u32*)c.chunk_k)[h] = add_sat(base, ex[k]);
        }
        base = add_sat(base, tot);
    }
    uint32_t empty = 0;
    for (int32_t f0 = 0; f0 < c.n; f0 += K) {
        uint32_t x[kMvIpl], ex[kMvIpl], tot;
#pragma unroll
        for (int k = 0; k < kMvIpl; ++k) {
            const int32_t f = f0 + ioff(k);
            x[k] = f < c.n && c.start(f + 1) <= c.start(f) ? 1u : 0u;
        }
        excl_scan4(sm, buf, x, ex, tot);
        empty += tot;
    }
    if (l == 0) {  // (the byte total of a well-formed column is within the capacity)
        res->n_empty = (int32_t)empty;
        res->n_bytes = (int64_t)min((int64_t)base, c.byte_cap);
    }
}

// one wave per column
__global__ __launch_bounds__(64 * kMvWaves) void mvt_scan_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, int64_t n_cols, uint8_t* __restrict__ out, covt_mvt_result* __restrict__ mres) {
    __shared__ AsmSmemT<1, kMvIpl> smem[kMvWaves];
    const int w = threadIdx.x >> 6;
    const int64_t col = uni64((int64_t)blockIdx.x * kMvWaves + w);
    if (col >= n_cols || mres[col].status != COVT_OK) return;
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, 0u, 0);
    mvt_scan_column<1>(c, mres + col, smem[w]);
}

// a workgroup per column (small batches)
__global__ __launch_bounds__(64 * kMvWaves) void mvt_scan_coop_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, int64_t n_cols, uint8_t* __restrict__ out, covt_mvt_result* __restrict__ mres) {
    __shared__ AsmSmemT<kMvWaves, kMvIpl> smem;
    const int64_t col = blockIdx.x;
    if (col >= n_cols || mres[col].status != COVT_OK) return;  // (uniform over the workgroup)
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, 0u, 0);
    mvt_scan_column<kMvWaves>(c, mres + col, smem);
}

// ---- 7. offsets ---------------------------------------------------------------------------------------
// blockIdx.x: the column; a thread per entry of offsets[0 .. n]
__global__ __launch_bounds__(64 * kMvWaves) void mvt_offsets_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, uint8_t* __restrict__ out, const covt_mvt_result* __restrict__ mres) {
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, 0u, 0);
    const int32_t n_bytes = (int32_t)mres[col].n_bytes;  // (launch 5's)
    const int32_t threads = (int32_t)(gridDim.y * 64 * kMvWaves);
    for (int32_t f = (int32_t)(blockIdx.y * 64 * kMvWaves + threadIdx.x); f <= c.n; f += threads) {
        int32_t o = n_bytes;
        const int32_t v = f < c.n && c.R > 0 ? c.start(f) : c.V;
        if (v < c.V) {
            // the last ring that starts at or before v: of the rings that start there the one with coordinates
            int32_t lo = 0, hi = c.R - 1;
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo + 1) / 2;
                if (c.ring_at(mid) <= v) lo = mid; else hi = mid - 1;
            }
            o = c.ring_at(lo + 1) > c.ring_at(lo) ? (int32_t)min(((g_u32*)c.ring_base)[lo], (uint32_t)n_bytes) : n_bytes;
        }
        ((gw_i32*)c.o_off)[f] = o;
    }
}

}  // namespace covt

extern "C" void covt_mvt_options_init(covt_mvt_options* opts) {
    if (!opts) return;
    opts->size = (uint32_t)sizeof(covt_mvt_options);
    opts->flags = 0;
    opts->shift = 0;
    opts->reserved = 0;
}

extern "C" int covt_geometry_mvt_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                        const covt_geom_result* d_gres, const covt_mvt_desc* d_mvdesc, int64_t n_columns,
                                        const covt_mvt_options* opts, uint8_t* d_mvt, covt_mvt_result* d_mvres,
                                        void* hip_stream) {
    using namespace covt;
    if (n_columns < 0 || !mvt_options_valid(opts) ||
        (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_mvdesc || !d_mvt || !d_mvres)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || d_asm == d_mvt) return COVT_ERR_INVALID_ARG;
    const uint32_t flags = opts->flags;  // (the options are read here, before the call returns)
    const int32_t shift = opts->shift;
    hipStream_t s = (hipStream_t)hip_stream;
    const unsigned cols256 = (unsigned)((n_columns + 255) / 256);
    const dim3 grid((unsigned)n_columns, product_blocks_y(n_columns)), block(64 * kMvWaves);
    hipLaunchKernelGGL(mvt_init_kernel, dim3(cols256), dim3(256), 0, s, d_gdesc, d_gres, d_mvdesc, n_columns, d_mvres);
    if (flags & COVT_MVT_ORIENT)
        hipLaunchKernelGGL(mvt_rings_kernel, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_mvdesc, flags, shift, d_mvt,
                           d_mvres);
    hipLaunchKernelGGL(mvt_features_kernel, grid, block, 0, s, d_decoded, d_gdesc, d_asm, d_gres, d_mvdesc, flags, shift,
                       d_mvt, d_mvres);
    hipLaunchKernelGGL(mvt_stream_kernel<false>, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_mvdesc, flags, shift, d_mvt,
                       d_mvres);
    if (n_columns <= kMvCoopMaxColumns)
        hipLaunchKernelGGL(mvt_scan_coop_kernel, dim3((unsigned)n_columns), block, 0, s, d_gdesc, d_asm, d_gres, d_mvdesc,
                           n_columns, d_mvt, d_mvres);
    else
        hipLaunchKernelGGL(mvt_scan_kernel, dim3((unsigned)((n_columns + kMvWaves - 1) / kMvWaves)), block, 0, s, d_gdesc,
                           d_asm, d_gres, d_mvdesc, n_columns, d_mvt, d_mvres);
    hipLaunchKernelGGL(mvt_stream_kernel<true>, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_mvdesc, flags, shift, d_mvt,
                       d_mvres);
    hipLaunchKernelGGL(mvt_offsets_kernel, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_mvdesc, d_mvt, d_mvres);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

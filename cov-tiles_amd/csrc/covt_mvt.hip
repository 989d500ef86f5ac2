// covt_mvt.hip -- gfx950 MVT geometry encoding of assembled geometry columns (include/covt.h "Geometry as MVT"):
// per feature the command stream of Feature.geometry (zigzag deltas, LEB128 varints) and its GeomType, in the
// column's slice of the mvt buffer.
//
// Seven launches (six without COVT_MVT_ORIENT); no allocation, no atomics, every output element written exactly
// once by one thread (so a captured graph replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the geometry's, then the layout's).
//   2. rings (COVT_MVT_ORIENT only): the segmented reduction of covt_segscan.h over the rings' edges (seg_run
//      under RingEdgePolicy), the value the int64 shoelace S_r over the shifted coordinates (MvEdge:
//      shoelace_term, the measures pass's policy); S_r goes to the upper half of the ring's record.
//   3. features: a thread per feature, the whole wave (a lane per ring, 64 rings a step) for those of kMvNarrow
//      rings or more.  It writes type[f] and walks the feature's rings in order; per ring it fixes k, whether the
//      ring is reversed, and the cursor predecessor: the source index of the last vertex the previous non-empty
//      ring of the feature emits, or -1 for the origin (the wave: a running maximum over the rings).  The record
//      {k, predecessor, flags, the feature's coordinate count} is all the coordinate passes need: an item is
//      local to its coordinate and its ring's record.
//   4. count: the coordinates in chunks of COVT_MVT_CHUNK, each with its ring and its predecessor (ring_stream
//      of covt_segscan.h), in output order: position a + j of the ring [a, b) is item j of the ring, which reads
//      source b - 1 - j if the ring is reversed; the position of a closed polygon ring's last coordinate is no
//      item.  An item's bytes are the commands in front of it (MoveTo before a ring's first item or a point
//      feature's first, LineTo before a ring's second), its two parameters and ClosePath after a polygon ring's
//      last.  The chunk's byte total goes to chunk_k[chunk].
//   5. scan: per column (a workgroup in small batches, a wave in large ones) the exclusive scan of chunk_k in
//      place -> n_bytes, and n_empty: the features without a coordinate (StepScan of covt_coop.h).
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
static_assert(COVT_MVT_RING_REC == 16, "a ring's record is four words");

// a ring's record: x = k, y = the cursor predecessor (a source index, -1: the origin), z = flags, w = the
// coordinate count of the point feature (kMvFirst); rings kernel: (z, w) = S_r until the features kernel
constexpr uint32_t kMvPoints = 1u;   // a ring of a POINT / MULTIPOINT feature: no commands of its own
constexpr uint32_t kMvFirst = 2u;    // the first non-empty ring of a point feature: MoveTo(w) in front
constexpr uint32_t kMvPolygon = 4u;  // ClosePath after the last item
constexpr uint32_t kMvRev = 8u;      // item j reads source b - 1 - j

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

// what the rings pass supplies to RingEdgePolicy: the shifted coordinates, shoelace_term, S_r into the upper half
// of the ring's record
struct MvEdge {
    typedef AddV<uint64_t> V;
    const MvCol& c;
    __device__ __forceinline__ int32_t map(int32_t v) const { return c.q(v); }
    __device__ __forceinline__ uint64_t edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) const {
        return shoelace_term(x0, y0, x1, y1);
    }
    __device__ __forceinline__ void put(int32_t r, uint64_t v, bool) const { ((gw_i64*)(c.rec + r))[1] = (int64_t)v; }
};
typedef RingEdgePolicy<MvEdge, kMvWaves> MvRings;

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
    __shared__ SegSmem<MvRings> sm;
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, flags, shift);
    const MvEdge e{c};
    MvRings p{c, e};
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
        wave_each(wide, [&](int src) {
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
        });
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

// blockIdx.x: the column; the walk is ring_stream's, the row here: the items' lengths, their inclusive scan
// over the row (its total the row's bytes) and, WRITE, the items' stores.
template <bool WRITE>
__global__ __launch_bounds__(64 * kMvWaves) void mvt_stream_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_mvt_desc* __restrict__ mdescs, uint32_t flags, int32_t shift, uint8_t* __restrict__ out,
    const covt_mvt_result* __restrict__ mres) {
    __shared__ __attribute__((aligned(16))) uint32_t marks[kMvWaves][128];
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;
    const MvCol c = mv_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, flags, shift);
    ring_stream<COVT_MVT_CHUNK, kMvWaves, WRITE>(
        c, c.chunk_k, marks[threadIdx.x >> 6], [&](int32_t v) { return c.q(v); }, [&](const RingRow& w) {
            const MvItem it0 = mv_item<WRITE>(c, w.i0 < w.B, w.i0, w.r0, w.x0, w.y0, w.bx, w.by);
            const MvItem it1 = mv_item<WRITE>(c, w.i0 + 1 < w.B, w.i0 + 1, w.r1, w.x1, w.y1, w.x0, w.y0);
            const uint32_t own = it0.len + it1.len;
            const uint32_t incl = incl_scan(own);
            if (WRITE) {
                const uint32_t d0 = w.run + incl - own, d1 = d0 + it0.len;
                mv_store(c, d0, it0);
                mv_store(c, d1, it1);
                // a ring's first position: the byte offset of the ring (offsets kernel)
                if (w.m0 != 0u && w.i0 < w.B) ((gw_u32*)c.ring_base)[w.m0 - 1u] = d0;
                if (w.m1 != 0u && w.i0 + 1 < w.B) ((gw_u32*)c.ring_base)[w.m1 - 1u] = d1;
            }
            return lane_bcast(incl, 63);
        });
}

// ---- 5. scan ------------------------------------------------------------------------------------------
// chunk_k -> its exclusive scan in place and n_bytes; n_empty
template <int NW>
__device__ void mvt_scan_column(const MvCol& c, covt_mvt_result* res, AsmSmemT<NW, kMvIpl>& sm) {
    const int l = Coop<NW, kMvIpl>::tid();
    StepScan<NW, kMvIpl> scan{sm};
    const uint32_t base = scan.in_place(c.chunk_k, ring_chunks<COVT_MVT_CHUNK>(c));
    const uint32_t empty = scan.sum(c.n, [&](int32_t f) { return c.start(f + 1) <= c.start(f) ? 1u : 0u; });
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

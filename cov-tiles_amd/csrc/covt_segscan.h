// covt_segscan.h -- what the per-column geometry products share on the device (covt_bbox.hip, covt_measures.hip,
// covt_simplify.hip, covt_mvt.hip; covt_wkb.hip uses the precheck and the launch sizing, covt_select.hip those
// and the 64-ary search): the clamped view of an assembled column, the status before any work, the workgroups per
// column, the segmented inclusive reduction over a column's items (below), its policy for per-ring sums over
// edges (RingEdgePolicy: measures, simplify, mvt), and the walk that hands every coordinate its ring
// (ring_stream: the count and write passes of simplify and mvt).
//
// The reduction.  A column's items (coordinates) fall into consecutive segments (features, rings), segment s
// being the range [start(s), start(s + 1)) with start nondecreasing; a value type with an associative join
// (ValueTrait below) is reduced per segment, every result handed once to one thread:
//
//   The items are cut into chunks of 128 * kRows; every wave of the column's gridDim.y workgroups takes a run
//   of consecutive chunks and owns the segments that start inside its run (an empty segment: where its start
//   falls; those at the column's end: the last run; a column without items is one chunk of none).  Per chunk
//   the wave loads its items once (two per lane and row), marks the chunk's segment heads in LDS, a lane per
//   segment, runs a segmented inclusive scan keyed on them over each row (DPP, carried from row to row and
//   chunk to chunk) into LDS, and a lane per segment that ends in the chunk picks the scan value of its last
//   item up and puts it.  Chunks that hold neither a head nor an item of one of the wave's segments are not
//   loaded.  The one segment still open at the end of the run is finished by its owner: by the wave if fewer
//   than kWide items remain, else by the whole workgroup through four hand-over slots in LDS once all its
//   waves are through their runs, the partial values joined in a fixed order (the run's carry, then waves
//   0 .. 3).  Every wave of the workgroup reaches the hand-over's barriers, whether its run was empty or not.
//
// A product is a ValueTrait and a Policy:
//
//   struct ValueTrait {
//       typedef ... T;
//       static T id();  static T join(T a, T b);  static T sel(bool p, T a, T b);    // p ? a : b
//       template <int CTRL, int RMASK> static T dpp(T old, T v);                     // dpp_move of every word
//       static T bcast(T v, int src);                                                // lane src's, uniform
//       template <int N> struct Lds { T get(int i) const;  void put(int i, T v); };  // N values in LDS
//   };
//   struct Policy {
//       typedef ValueTrait V;
//       static constexpr int kWaves, kRows, kWide;
//       static constexpr int kIncl;   // heads_inclusive_end: 1 if an item's term depends on whether the *next*
//                                     // item is a head, so heads are marked at 0 .. L (start(count()) too)
//       static constexpr int kAhead;  // starts wanted readable past the first open segment at a chunk's top
//       int32_t count() const, items() const;        // segments, items
//       int32_t first_at(int32_t x);                 // the first segment s in [0, count()] with start(s) >= x
//       void open(int32_t s);                        // before the first chunk: s the run's first segment
//       void ensure(int32_t s, int32_t need);        // makes start(s .. s + need - 1) readable (uniform)
//       int32_t start(int32_t s);                    // per lane; past count(): INT32_MAX
//       struct Raw;  void load(Raw&, int32_t a, int32_t b);   // the chunk [a, b)'s items, before the heads
//       void terms(const Raw&, int k, int32_t a, int32_t p0, int32_t L, int32_t h1, int32_t h2, T& c0, T& c1);
//           // the terms of items p0, p0 + 1 of the chunk (row k; id() from L on); h1, h2: the head flags of
//           // items p0 + 1 and (kIncl) p0 + 2
//       T tail(int32_t from, int32_t to, int32_t tid, int32_t threads);   // thread tid's share of [from, to)
//       void put(int32_t s, T v, bool any);          // segment s's result (any: it has an item)
//   };
#ifndef COVT_SEGSCAN_H
#define COVT_SEGSCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_coop.h"
#include "covt_wave.h"

namespace covt {

// ---- launch sizing ------------------------------------------------------------------------------------
// workgroups per column of a product's main kernel: 8192 over all columns of a small batch, at most 64 each
// (a 72k-coordinate column: a chunk or two per wave)
inline unsigned product_blocks_y(int64_t n_columns) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, 8192 / n_columns));
}

// ---- the column ---------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t clamp0(int32_t x, int32_t hi) { return min(max(x, 0), hi); }

// An assembled column: n features -> P parts -> R rings -> V coordinates by nested absolute offsets.  The
// counts are clamped to the slices' capacities and every offset read is clamped to the next level's count, so
// a column whose offsets are not what assembly promises is still read inside its slices.
struct GeomCol {
    const int32_t *geo, *part, *ring, *xy;
    int32_t n, P, R, V;

    __device__ __forceinline__ int32_t geo_at(int32_t f) const { return clamp0(((const g_i32*)geo)[f], P); }
    __device__ __forceinline__ int32_t part_at(int32_t g) const { return clamp0(((const g_i32*)part)[g], R); }
    __device__ __forceinline__ int32_t ring_at(int32_t r) const { return clamp0(((const g_i32*)ring)[r], V); }
    // first coordinate of feature f in [0, n] (start(n): the column's coordinate count)
    __device__ __forceinline__ int32_t start(int32_t f) const { return ring_at(part_at(geo_at(f))); }
    // coordinate i (below V) as (x, y)
    __device__ __forceinline__ void load1(int32_t i, int32_t& x, int32_t& y) const {
        const uint64_t v = *(g_u64*)(xy + 2 * (int64_t)i);
        x = (int32_t)(uint32_t)v;
        y = (int32_t)(uint32_t)(v >> 32);
    }
    // coordinates i, i + 1 (i even: 16-byte aligned) as (x0, y0, x1, y1); those at or past `end` are not read
    __device__ __forceinline__ i32x4 load2(int32_t i, int32_t end) const {
        i32x4 q = i32x4{0, 0, 0, 0};
        if (i + 1 < end) {
            q = *(g_i32x4*)(xy + 2 * (int64_t)i);
        } else if (i < end) {
            int32_t x, y;
            load1(i, x, y);
            q.x = x, q.y = y;
        }
        return q;
    }
};
__device__ __forceinline__ GeomCol geom_col(const covt_geom_desc& gd, const covt_geom_result& gr, const uint8_t* asmb,
                                            int32_t n_features) {
    GeomCol c;
    c.geo = (const int32_t*)(asmb + gd.out_off[0]);
    c.part = (const int32_t*)(asmb + gd.out_off[1]);
    c.ring = (const int32_t*)(asmb + gd.out_off[2]);
    c.xy = (const int32_t*)(asmb + gd.out_off[3]);
    c.n = n_features;
    c.P = clamp0(gr.num_parts, gd.part_cap);
    c.R = clamp0(gr.num_rings, gd.ring_cap);
    c.V = clamp0(gr.num_coords, gd.coord_cap);
    return c;
}

// The int64 policy of a ring's doubled signed area S_r (include/covt.h "Geometry measures"; the winding of
// "Geometry as MVT"): the edge from (x0, y0) to (x1, y1) adds x0 * y1 - x1 * y0, every product exact in int64,
// the sum taken mod 2^64.
__host__ __device__ __forceinline__ uint64_t shoelace_term(int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    return (uint64_t)((int64_t)x0 * (int64_t)y1) - (uint64_t)((int64_t)x1 * (int64_t)y0);
}

// a product column's status before any work: that of the pass it reads (`upstream`), then the layout's
// (too_large, off_ok: the descriptors' flags and offsets; n_ok: planned for the rows its input has)
__device__ __forceinline__ int32_t product_precheck(int32_t upstream, bool too_large, bool off_ok, bool n_ok) {
    if (upstream != COVT_OK) return upstream;
    if (too_large || !off_ok) return COVT_ERR_INVALID_ARG;
    return n_ok ? COVT_OK : COVT_ERR_INVALID_ARG;
}

// the same for a product of the assembly (too_large, off_ok: the product's own descriptor; n_features: what it
// was planned for)
__device__ __forceinline__ int32_t geom_product_precheck(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                         bool too_large, bool off_ok, int32_t n_features) {
    const int32_t n = gd.in_off[0] >= 0 ? gd.in_len[0] : 0;  // the features the assembly walked
    return product_precheck(gr.status, ((uint32_t)gd.flags & COVT_GEOM_TOO_LARGE) || too_large, off_ok, n_features == n);
}

// the first i in [0, n] with start(i) >= x (start nondecreasing over [0, n)): the wave probes 64 evenly
// spaced i per step (x uniform)
template <class Start>
__device__ __forceinline__ int32_t seg_first_at(int32_t n, int32_t x, Start start) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t step = (hi - lo + 63) >> 6;
        const int32_t p = min(lo + lane_id() * step, hi);
        const bool below = p < hi && start(p) < x;  // (a prefix of the lanes)
        const int cnt = __popcll(__ballot(below));
        if (cnt == 0) {
            hi = lo;
        } else {
            const int32_t nlo = min(lo + (cnt - 1) * step, hi) + 1;
            hi = cnt < 64 ? min(lo + cnt * step, hi) : hi;
            lo = nlo;
        }
    }
    return uni(lo);
}

// ---- scans and reductions of a value trait ------------------------------------------------------------
// one step of the segmented inclusive scan: (v, f) := (pv, pf) (+) (v, f); a lane with f set starts a segment
// (selects, not branches: the DPP moves run with every lane enabled)
template <class V>
struct SegScanStep {
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ void step(typename V::T& v, int32_t& f) {
        const typename V::T pv = V::template dpp<CTRL, RMASK>(V::id(), v);
        const int32_t pf = (int32_t)dpp_move<CTRL, RMASK>(0u, (uint32_t)f);
        v = V::sel(f != 0, v, V::join(pv, v));
        f |= pf;
    }
};
template <class V>
struct SegRedStep {
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ void step(typename V::T& v) {
        v = V::join(V::template dpp<CTRL, RMASK>(V::id(), v), v);
    }
};
// the join of the 64 lanes' values in the fixed order of the wave64 DPP sequence, uniform
template <class V>
__device__ __forceinline__ typename V::T seg_wave_join(typename V::T v) {
    wave_dpp_seq<SegRedStep<V>>(v);
    return V::bcast(v, 63);
}
// One row of a chunk: the lane holds the terms c0, c1 of two consecutive items (id() past the column's end)
// and their head flags; `carry` is the running value of the segment open before lane 0 (uniform).
// r0, r1: the inclusive segmented join at the two items; carry: that at the row's last one.
template <class V>
__device__ __forceinline__ void seg_row_scan(typename V::T c0, typename V::T c1, int32_t h0, int32_t h1,
                                             typename V::T& carry, typename V::T& r0, typename V::T& r1) {
    typename V::T v = V::sel(h1 != 0, c1, V::join(c0, c1));
    int32_t f = h0 | h1;
    v = V::sel(lane_id() == 0 && f == 0, V::join(carry, v), v);
    wave_dpp_seq<SegScanStep<V>>(v, f);
    const typename V::T ex = V::template dpp<0x138, 0xf>(carry, v);  // wave_shr:1: the lane before (lane 0: the carry)
    r0 = V::sel(h0 != 0, c0, V::join(ex, c0));
    r1 = V::sel(h1 != 0, c1, V::join(r0, c1));
    carry = V::bcast(v, 63);
}

// a sum mod 2^32 or 2^64 (U: uint32_t, uint64_t) under addition
template <class U>
struct AddV {
    typedef U T;
    static __device__ __forceinline__ T id() { return 0; }
    static __device__ __forceinline__ T join(T a, T b) { return a + b; }
    static __device__ __forceinline__ T sel(bool p, T a, T b) { return p ? a : b; }
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ T dpp(T old, T v) {
        return dpp_move<CTRL, RMASK>(old, v);
    }
    static __device__ __forceinline__ T bcast(T v, int src) {
        if constexpr (sizeof(U) == 8) return lane_bcast64(v, src);
        else return lane_bcast(v, src);
    }
    template <int N>
    struct Lds {
        U v[N];
        __device__ __forceinline__ T get(int i) const { return v[i]; }
        __device__ __forceinline__ void put(int i, T x) { v[i] = x; }
    };
};

// zero the wave's N head bytes (N a multiple of 4), four a lane and step
template <int N>
__device__ __forceinline__ void seg_clear_heads(uint8_t* head) {
#pragma unroll
    for (int i = 0; i < N; i += 256)
        if (N - i >= 256 || 4 * lane_id() < N - i) *(uint32_t*)(head + i + 4 * lane_id()) = 0;
}

// ---- the run ------------------------------------------------------------------------------------------
template <class P>
struct __attribute__((aligned(16))) SegSmem {
    static constexpr int kChunk = 128 * P::kRows;
    static constexpr int kHead = kChunk + 4 * P::kIncl;
    typename P::V::template Lds<kChunk> res[P::kWaves];  // the chunk's inclusive segmented join per item
    uint8_t head[P::kWaves][kHead];                      // 1: a segment starts at this item of the chunk
    typename P::V::template Lds<P::kWaves> wide;         // a wave's segment left to the workgroup: its value so far,
    int32_t wide_seg[P::kWaves];                         //   its index (-1: none),
    int32_t wide_from[P::kWaves];                        //   and the items [from, to) still to take
    int32_t wide_to[P::kWaves];
    typename P::V::template Lds<P::kWaves> red;
};

// blockIdx.x: the column; each of its gridDim.y * kWaves waves takes a run of consecutive chunks.  Called by
// every thread of the workgroup (its barriers); the policy is the wave's.
template <class P>
__device__ __forceinline__ void seg_run(P& p, SegSmem<P>& sm) {
    typedef typename P::V V;
    typedef typename V::T T;
    constexpr int kChunk = SegSmem<P>::kChunk, kHead = SegSmem<P>::kHead, kIncl = P::kIncl;
    const int l = lane_id();
    const int w = threadIdx.x >> 6;
    const int32_t wave = uni((int32_t)(blockIdx.y * P::kWaves + w));
    const int32_t waves = (int32_t)(gridDim.y * P::kWaves);
    const int32_t n = p.count(), N = p.items();
    // (a column without items is one chunk of none: its segments are all empty)
    const int64_t chunks = std::max<int64_t>(1, ((int64_t)N + kChunk - 1) / kChunk);
    const int32_t cb = (int32_t)(chunks * wave / waves), ce = (int32_t)(chunks * (wave + 1) / waves);
    int32_t wide_seg = -1, wide_from = 0, wide_to = 0;
    T carry = V::id();
    if (cb < ce && n > 0) {
        auto& res = sm.res[w];
        uint8_t* const head = sm.head[w];
        const bool last = ce == chunks;  // the column's last run: owns the empty segments at its end
        const int32_t A = cb * kChunk, B = last ? N : ce * kChunk;
        int32_t sc = A == 0 ? 0 : p.first_at(A);  // the first segment not yet put
        seg_clear_heads<kHead>(head);
        p.open(sc);
        wave_sync();
        for (int32_t j = cb; j < ce && sc < n; ++j) {
            const int32_t a = j * kChunk, L = min(kChunk, N - a), b = a + L;
            p.ensure(sc, P::kAhead);
            const int32_t s_sc = uni(p.start(sc));
            if (!last && s_sc >= B) break;  // the next segment starts in a later run
            const bool process = s_sc < b;  // a segment of this wave's has an item here
            if (!process && j != chunks - 1) continue;
            if (process) {
                typename P::Raw raw;
                p.load(raw, a, b);
                // heads: the segments from sc on that start below b (kIncl: at or below; start(n) is the column's end)
                for (int32_t sh = sc;; sh += 64) {
                    p.ensure(sh, 64);
                    const int32_t s = sh + l;
                    const int32_t st = p.start(s);
                    const bool in = kIncl ? s <= n && st <= b : s < n && st < b;
                    if (in && (kIncl ? (uint32_t)(st - a) <= (uint32_t)L : (uint32_t)(st - a) < (uint32_t)L)) head[st - a] = 1;
                    if (__ballot(in) != ~0ull) break;
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < P::kRows; ++k) {
                    const int32_t p0 = 128 * k + 2 * l;
                    const uint32_t hh = *(const uint16_t*)(head + p0);
                    const int32_t h0 = (int32_t)(hh & 0xffu), h1 = (int32_t)(hh >> 8);
                    const int32_t h2 = kIncl ? head[p0 + 2] : 0;
                    T c0, c1, r0, r1;
                    p.terms(raw, k, a, p0, L, h1, h2, c0, c1);
                    seg_row_scan<V>(c0, c1, h0, h1, carry, r0, r1);
                    res.put(p0, r0);
                    res.put(p0 + 1, r1);
                }
                wave_sync();
                seg_clear_heads<kHead>(head);  // (read above)
            }
            // the segments that end in this chunk: a lane each, in steps of 64
            for (;;) {
                p.ensure(sc, 65);
                const int32_t s = sc + l;
                const int32_t st = p.start(s), e = p.start(s + 1);
                const bool done = s < n && (last || st < B) && e <= b;  // (a prefix of the lanes)
                if (done) {
                    const uint32_t at = (uint32_t)(e - 1 - a);
                    const bool any = e > st && process && at < (uint32_t)kChunk;
                    p.put(s, any ? res.get(at) : V::id(), any);
                }
                const int cnt = __popcll(__ballot(done));
                sc += cnt;
                if (cnt < 64) break;
            }
            wave_sync();  // (res and head are rewritten by the next chunk)
        }
        // the segment still open at the end of the run: the items [B, e) are left
        if (!last && sc < n) {
            p.ensure(sc, 2);
            const int32_t st = uni(p.start(sc)), e = uni(p.start(sc + 1));
            if (st < B && e > B) {
                if (e - B >= P::kWide) {
                    wide_seg = sc, wide_from = B, wide_to = e;
                } else {
                    const T v = V::join(carry, seg_wave_join<V>(p.tail(B, e, l, 64)));
                    if (l == 0) p.put(sc, v, true);
                }
            }
        }
    }
    if (l == 0) {
        sm.wide_seg[w] = wide_seg;
        sm.wide_from[w] = wide_from;
        sm.wide_to[w] = wide_to;
        sm.wide.put(w, carry);
    }
    __syncthreads();
    // segments left to the workgroup: all its threads take the remaining items, then the waves' values in wave order
    for (int k = 0; k < P::kWaves; ++k) {
        const int32_t s = sm.wide_seg[k];
        if (s < 0) continue;  // (uniform)
        T v = seg_wave_join<V>(p.tail(sm.wide_from[k], sm.wide_to[k], (int32_t)threadIdx.x, 64 * P::kWaves));
        if (l == 0) sm.red.put(w, v);
        __syncthreads();
        if (threadIdx.x == 0) {
            v = sm.wide.get(k);
#pragma unroll
            for (int i = 0; i < P::kWaves; ++i) v = V::join(v, sm.red.get(i));
            p.put(s, v, true);
        }
        __syncthreads();
    }
}

// ---- the rings of a column as segments ------------------------------------------------------------------
// The policy of a per-ring sum over edges: the segments are the rings of a GeomCol, read from ring[] directly;
// a chunk is one row of 128 coordinates (16 bytes a lane); a coordinate's term is that of its edge to the next
// coordinate -- the lane takes it from its neighbour (DPP) -- and id() where the next coordinate starts another
// ring or the column ends (so heads are marked up to and including the chunk's end).  The product is
//
//   struct Edge {
//       typedef ValueTrait V;
//       int32_t map(int32_t v) const;                                      // applied to every coordinate read
//       V::T edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) const;   // of mapped coordinates
//       void put(int32_t r, V::T v, bool any) const;                       // ring r's sum (any: it has a coordinate)
//   };
template <class Edge, int WAVES>
struct RingEdgePolicy {
    typedef typename Edge::V V;
    typedef typename V::T T;
    static constexpr int kWaves = WAVES;
    static constexpr int kRows = 1;
    static constexpr int kWide = 2048;  // coordinates left past a run from which the workgroup finishes a ring
    static constexpr int kIncl = 1;     // an edge's term depends on whether the next coordinate is a head
    static constexpr int kAhead = 1;
    struct Raw {
        i32x4 q;         // mapped
        int32_t tx, ty;  // the coordinate after the chunk, mapped (uniform)
    };

    const GeomCol& c;
    const Edge& e;

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
        r.q = i32x4{e.map(q.x), e.map(q.y), e.map(q.z), e.map(q.w)};
        r.tx = r.ty = 0;
        if (b < c.V) {
            c.load1(b, r.tx, r.ty);
            r.tx = e.map(r.tx), r.ty = e.map(r.ty);
        }
    }
    __device__ __forceinline__ void terms(const Raw& r, int, int32_t a, int32_t p0, int32_t L, int32_t h1, int32_t h2,
                                          T& t0, T& t1) const {
        // the coordinate after this lane's two: the next lane's first (lane 63: the one after the chunk)
        const int32_t nx = (int32_t)lane_next((uint32_t)r.q.x, (uint32_t)r.tx);
        const int32_t ny = (int32_t)lane_next((uint32_t)r.q.y, (uint32_t)r.ty);
        const T e0 = e.edge(r.q.x, r.q.y, r.q.z, r.q.w), e1 = e.edge(r.q.z, r.q.w, nx, ny);
        t0 = V::sel(a + p0 + 1 < c.V && h1 == 0 && p0 + 1 < L, e0, V::id());
        t1 = V::sel(a + p0 + 2 < c.V && h2 == 0 && p0 + 1 < L, e1, V::id());
    }
    // the edges from the coordinates [from, to - 1)
    __device__ __forceinline__ T tail(int32_t from, int32_t to, int32_t tid, int32_t threads) const {
        T part = V::id();
        for (int32_t i = from + tid; i + 1 < to; i += threads) {
            int32_t x0, y0, x1, y1;
            c.load1(i, x0, y0);
            c.load1(i + 1, x1, y1);
            part = V::join(part, e.edge(e.map(x0), e.map(y0), e.map(x1), e.map(y1)));
        }
        return part;
    }
    __device__ __forceinline__ void put(int32_t r, T v, bool any) const { e.put(r, v, any); }
};

// ---- the ring of every coordinate -----------------------------------------------------------------------
// chunks of CHUNK coordinates of a column's count and write passes (a column without rings has no item)
template <int CHUNK>
__device__ __forceinline__ int32_t ring_chunks(const GeomCol& c) {
    return c.R > 0 ? (int32_t)(((int64_t)c.V + CHUNK - 1) / CHUNK) : 0;
}

// what a row's callback gets: the lane's two positions and what the walk knows of them
struct RingRow {
    int32_t i0, B;           // the positions i0, i0 + 1 (those at or past the chunk's end B are none)
    int32_t r0, r1;          // their rings (in 0 .. R - 1)
    uint32_t m0, m1;         // their marks: ring + 1 at the first position of a non-empty ring, else 0
    int32_t x0, y0, x1, y1;  // their coordinates, mapped
    int32_t bx, by;          // the coordinate before i0, mapped (i0 + 1's is (x0, y0))
    uint32_t run;            // the chunk's base plus what the rows before advanced it by (uniform)
};

// A column's coordinates in chunks of CHUNK, a wave per chunk, the column's gridDim.y * WAVES waves striding over
// them, a row of 128 at a time, two consecutive positions a lane: row(RingRow) is called by the whole wave once
// per row and returns what the row adds to `run` (uniform).  `run` starts at 0 and the chunk's total goes to
// chunk_k[chunk] (the count pass), or WRITE: it starts at chunk_k[chunk], by then its exclusive scan.  map is
// applied to every coordinate.  `mark` is the wave's 128 words of LDS.
//
// The ring of the chunk's first coordinate comes from the 64-ary search; per row the rings that start in it are
// marked in LDS, a lane per ring, and a coordinate's ring is the running maximum of the marks up to it (DPP),
// carried from row to row in `open`; its predecessor comes by DPP too.  What this rests on:
//   - a mark is ring + 1 at the start of a *non-empty* ring, so there is one ring per position and the maximum
//     is the position's own ring; rlo, the last ring that starts at or before the chunk, may be empty or start
//     at the chunk's first position itself, so the marking starts from it;
//   - the lane clears its two marks as it reads them; the next row's marks (and the next chunk's) follow the
//     wave_sync at the row's end, the reads follow the wave_sync after the marking;
//   - sc, open, run, px and py are wave-uniform, so every branch on them is, and the DPP moves and the ballots
//     of the walk and of the callback run with the whole wave active.
template <int CHUNK, int WAVES, bool WRITE, class Map, class Row>
__device__ __forceinline__ void ring_stream(const GeomCol& c, uint32_t* chunk_k, uint32_t* mark, Map map, Row row) {
    static_assert(CHUNK % 128 == 0, "a chunk is whole rows");
    const int l = lane_id();
    const int32_t chunks = ring_chunks<CHUNK>(c);
    const auto ring_at = [&](int32_t r) { return c.ring_at(r); };
    *(uint64_t*)(mark + 2 * l) = 0ull;
    wave_sync();
    for (int32_t ch = uni((int32_t)(blockIdx.y * WAVES + (threadIdx.x >> 6))); ch < chunks;
         ch += (int32_t)(gridDim.y * WAVES)) {
        const int32_t A = ch * CHUNK, B = min(A + CHUNK, c.V);
        // the ring of the chunk's first coordinate: the last one that starts at or before it
        const int32_t rlo = clamp0(seg_first_at(c.R, A + 1, ring_at) - 1, c.R - 1);
        uint32_t open = (uint32_t)rlo + 1u;  // ring + 1 of the coordinate before the row
        int32_t sc = rlo;                    // the first ring not yet marked
        uint32_t run = WRITE ? (uint32_t)uni((int32_t)((g_u32*)chunk_k)[ch]) : 0u;
        int32_t px = 0, py = 0;  // the coordinate before the row, mapped
        if (A > 0) {
            c.load1(A - 1, px, py);
            px = map(px), py = map(py);
        }
        for (int k = 0; k < CHUNK / 128; ++k) {
            const int32_t a = A + 128 * k, b = min(a + 128, B), i0 = a + 2 * l;
            if (a >= B) break;
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
            *(uint64_t*)(mark + 2 * l) = 0ull;
            const uint32_t m0 = (uint32_t)mm, m1 = (uint32_t)(mm >> 32);
            const uint32_t inc = incl_max_scan(max(m0, m1));
            // the maximum over the lanes before (wave_shr:1), the rows before (open) and the lane's own marks
            const uint32_t r0 = max(max(dpp_move<0x138, 0xf>(0u, inc), open), m0), r1 = max(r0, m1);
            open = max(open, lane_bcast(inc, 63));
            const int32_t x0 = map(q.x), y0 = map(q.y), x1 = map(q.z), y1 = map(q.w);
            // the coordinate before this lane's two: the lane before's second (lane 0: the one before the row)
            const int32_t bx = (int32_t)dpp_move<0x138, 0xf>((uint32_t)px, (uint32_t)x1);
            const int32_t by = (int32_t)dpp_move<0x138, 0xf>((uint32_t)py, (uint32_t)y1);
            px = (int32_t)lane_bcast((uint32_t)x1, 63), py = (int32_t)lane_bcast((uint32_t)y1, 63);
            // (r0, r1 are in 1 .. R: open is, and so is every mark)
            run += row(RingRow{i0, B, (int32_t)r0 - 1, (int32_t)r1 - 1, m0, m1, x0, y0, x1, y1, bx, by, run});
            wave_sync();
        }
        if (!WRITE && l == 0) ((gw_u32*)chunk_k)[ch] = run;
    }
}

}  // namespace covt

#endif

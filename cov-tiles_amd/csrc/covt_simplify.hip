// covt_simplify.hip -- gfx950 geometry simplification of assembled geometry columns (include/covt.h "Geometry
// simplification"): snap to the grid of 2^s, drop the coordinates that repeat their predecessor, empty the rings
// and lines that collapsed; the output is another assembled column in the simplify buffer.
//
// Six launches; no allocation, no atomics, every output element written exactly once by one thread (so a
// captured graph replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's and the shift's), its part and ring counts.
//   2. rings: the segmented reduction of covt_segscan.h under KeepPolicy: the segments are the rings, the value
//      a count, a chunk one row of 128 coordinates (16 bytes a lane), and a coordinate's term is 1 if the next
//      coordinate is in the same ring and snaps differently -- the lane takes it from its neighbour (DPP).  A
//      non-empty ring's k_r = 1 + the sum goes to ring_k[r] in the column's scratch.
//   3. features: a thread per feature, the whole wave (a lane per part) for those of kSpNarrow parts or rings.
//      It applies the type minima and the shell rule part by part and stores k'_r over k_r, bit 31 set for
//      the rings of POINT / MULTIPOINT features (k'_r their length: every coordinate is kept).
//   4. count: the coordinates in chunks of COVT_SIMPLIFY_CHUNK, a wave per chunk, a row of 128 at a time.  The ring
//      of the chunk's first coordinate by the 64-ary search; per row the rings that start in it marked in LDS, a
//      lane per ring, and every coordinate's ring the running maximum of the marks (DPP), its predecessor by DPP
//      too; kept iff its ring stands and it is a point, its ring's first or differs from its predecessor.  The
//      chunk's kept count goes to chunk_k[chunk].
//   5. scan: per column (a workgroup in small batches, a wave in large ones) the exclusive scan of k'_r ->
//      ring_offsets' and num_coords, the exclusive scan of chunk_k in place, the copy of the two upper levels.
//   6. write: pass 4 again; a kept coordinate's destination is its chunk's base plus its rank in the chunk
//      (ballots), which is ring_offsets'[r] plus its rank among its ring's kept coordinates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt.h"
#include "covt_segscan.h"
#include "covt_simplify_plan.h"

namespace covt {

constexpr int kSpWaves = 4;                // waves per workgroup
constexpr int kSpNarrow = 64;              // rings or parts from which a feature is finished by the whole wave
constexpr int kSpIpl = 4;                  // scan: items per thread and step
constexpr int kSpCoopMaxColumns = 4096;    // scan: batches of at most this many columns get a workgroup per column
constexpr int kSpRows = COVT_SIMPLIFY_CHUNK / 128;  // count / write: rows of 128 coordinates per chunk
constexpr uint32_t kSpPoints = 0x80000000u;         // ring_k: a ring of a POINT / MULTIPOINT feature
static_assert(COVT_SIMPLIFY_CHUNK % 128 == 0, "a chunk is whole rows");

typedef __attribute__((address_space(1))) uint32_t gw_u32;
typedef __attribute__((address_space(1))) int32_t gw_i32;
typedef __attribute__((address_space(1))) uint64_t gw_u64;

// a count under addition
struct CntV {
    typedef uint32_t T;
    static __device__ __forceinline__ T id() { return 0u; }
    static __device__ __forceinline__ T join(T a, T b) { return a + b; }
    static __device__ __forceinline__ T sel(bool p, T a, T b) { return p ? a : b; }
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ T dpp(T old, T v) {
        return dpp_move<CTRL, RMASK>(old, v);
    }
    static __device__ __forceinline__ T bcast(T v, int src) { return lane_bcast(v, src); }
    template <int N>
    struct Lds {
        uint32_t v[N];
        __device__ __forceinline__ T get(int i) const { return v[i]; }
        __device__ __forceinline__ void put(int i, T x) { v[i] = x; }
    };
};

struct SpCol : GeomCol {
    const uint8_t* types;
    int32_t *o_geo, *o_part, *o_ring, *o_xy;  // the simplified column
    uint32_t *ring_k, *chunk_k;               // the scratch
    int32_t coord_cap;
    int32_t s;  // the shift

    __device__ __forceinline__ int32_t snap(int32_t v) const { return simplify_snap(v, s); }
    // chunks of the count and write passes (a column without rings keeps nothing)
    __device__ __forceinline__ int32_t chunks() const {
        return R > 0 ? (int32_t)(((int64_t)V + COVT_SIMPLIFY_CHUNK - 1) / COVT_SIMPLIFY_CHUNK) : 0;
    }
};
__device__ __forceinline__ SpCol sp_column(const covt_geom_desc& gd, const covt_geom_result& gr,
                                           const covt_simplify_desc& sd, const uint8_t* dec, const uint8_t* asmb,
                                           uint8_t* out, int32_t shift) {
    SpCol c;
    (GeomCol&)c = geom_col(gd, gr, asmb, sd.n_features);
    c.types = dec ? dec + gd.in_off[0] : nullptr;  // (only the features kernel reads types)
    uint8_t* const o = out + sd.off;
    c.o_geo = (int32_t*)(o + simplify_geo_off(sd.n_features));
    c.o_part = (int32_t*)(o + simplify_part_off(sd.n_features));
    c.o_ring = (int32_t*)(o + simplify_ring_off(sd.n_features, sd.part_cap));
    c.o_xy = (int32_t*)(o + simplify_coords_off(sd.n_features, sd.part_cap, sd.ring_cap));
    c.ring_k = (uint32_t*)(o + simplify_ring_k_off(sd.n_features, sd.part_cap, sd.ring_cap, sd.coord_cap));
    c.chunk_k = (uint32_t*)(o + simplify_chunk_k_off(sd.n_features, sd.part_cap, sd.ring_cap, sd.coord_cap));
    c.coord_cap = sd.coord_cap;
    c.s = shift;
    return c;
}
__device__ __forceinline__ int32_t sp_shift(int32_t shift, const int32_t* __restrict__ d_shift, int64_t col) {
    return d_shift ? d_shift[col] : shift;
}

// The rings of a column as the segments of covt_segscan.h, the value the number of coordinates that differ from
// their predecessor in the same ring.
struct KeepPolicy {
    typedef CntV V;
    static constexpr int kWaves = kSpWaves;
    static constexpr int kRows = 1;     // one row of 64 lanes x 2 coordinates per chunk: 128 coordinates
    static constexpr int kWide = 2048;  // coordinates left past a run from which the workgroup finishes a ring
    static constexpr int kIncl = 1;     // a coordinate's term depends on whether the next coordinate is a head
    static constexpr int kAhead = 1;
    struct Raw {
        i32x4 q;         // snapped
        int32_t tx, ty;  // the coordinate after the chunk, snapped (uniform)
    };

    const SpCol& c;

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
        r.q = i32x4{c.snap(q.x), c.snap(q.y), c.snap(q.z), c.snap(q.w)};
        r.tx = r.ty = 0;
        if (b < c.V) {
            c.load1(b, r.tx, r.ty);
            r.tx = c.snap(r.tx), r.ty = c.snap(r.ty);
        }
    }
    __device__ __forceinline__ void terms(const Raw& r, int, int32_t a, int32_t p0, int32_t L, int32_t h1, int32_t h2,
                                          uint32_t& t0, uint32_t& t1) const {
        // the coordinate after this lane's two: the next lane's first (lane 63: the one after the chunk)
        const int32_t nx = (int32_t)lane_next((uint32_t)r.q.x, (uint32_t)r.tx);
        const int32_t ny = (int32_t)lane_next((uint32_t)r.q.y, (uint32_t)r.ty);
        const bool d0 = r.q.x != r.q.z || r.q.y != r.q.w, d1 = r.q.z != nx || r.q.w != ny;
        t0 = a + p0 + 1 < c.V && h1 == 0 && p0 + 1 < L && d0 ? 1u : 0u;
        t1 = a + p0 + 2 < c.V && h2 == 0 && p0 + 1 < L && d1 ? 1u : 0u;
    }
    // the terms of the coordinates [from, to - 1)
    __device__ __forceinline__ uint32_t tail(int32_t from, int32_t to, int32_t tid, int32_t threads) const {
        uint32_t part = 0;
        for (int32_t i = from + tid; i + 1 < to; i += threads) {
            int32_t x0, y0, x1, y1;
            c.load1(i, x0, y0);
            c.load1(i + 1, x1, y1);
            part += c.snap(x0) != c.snap(x1) || c.snap(y0) != c.snap(y1) ? 1u : 0u;
        }
        return part;
    }
    __device__ __forceinline__ void put(int32_t r, uint32_t v, bool any) const {
        ((gw_u32*)c.ring_k)[r] = any ? v + 1u : 0u;
    }
};

// ---- 1. init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void simplify_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                            const covt_geom_result* __restrict__ gres,
                                                            const covt_simplify_desc* __restrict__ sdescs,
                                                            int64_t n_cols, const int32_t* __restrict__ d_shift,
                                                            covt_geom_result* __restrict__ ores) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    int32_t* r = (int32_t*)(ores + c);
    const covt_simplify_desc sd = sdescs[c];
    const covt_geom_desc gd = gdescs[c];
    const covt_geom_result gr = gres[c];
    int32_t st = geom_product_precheck(gd, gr, (sd.flags & COVT_SIMPLIFY_TOO_LARGE) != 0, sd.off >= 0 && !(sd.off & 15),
                                       sd.n_features);
    if (st == COVT_OK && (sd.part_cap != gd.part_cap || sd.ring_cap != gd.ring_cap || sd.coord_cap != gd.coord_cap))
        st = COVT_ERR_INVALID_ARG;
    if (st == COVT_OK && d_shift && !simplify_shift_valid(d_shift[c])) st = COVT_ERR_INVALID_ARG;
    r[0] = st;
    if (st == COVT_OK) {  // (num_coords: the scan's)
        r[1] = clamp0(gr.num_parts, gd.part_cap);
        r[2] = clamp0(gr.num_rings, gd.ring_cap);
    } else {
        r[1] = r[2] = r[3] = 0;
    }
}

// ---- 2. rings -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kSpWaves) void simplify_rings_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_simplify_desc* __restrict__ sdescs, int32_t shift, const int32_t* __restrict__ d_shift,
    uint8_t* __restrict__ out, const covt_geom_result* __restrict__ ores) {
    __shared__ SegSmem<KeepPolicy> sm;
    const int64_t col = blockIdx.x;
    if (ores[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, sp_shift(shift, d_shift, col));
    KeepPolicy p{c};
    seg_run(p, sm);
}

// ---- 3. features --------------------------------------------------------------------------------------
// the rings of part g of a feature of type t: k_r -> k'_r
__device__ __forceinline__ void sp_part(const SpCol& c, int32_t g, uint32_t t) {
    const int32_t r0 = c.part_at(g), r1 = c.part_at(g + 1);
    const bool points = t == 0u || t == 3u, line = t == 1u || t == 4u, polygon = t == 2u || t == 5u;
    bool shell_gone = false;
    for (int32_t r = r0; r < r1; ++r) {
        uint32_t k = points ? (uint32_t)max(c.ring_at(r + 1) - c.ring_at(r), 0) : ((g_u32*)c.ring_k)[r];
        if (line && k < 2u) k = 0u;
        if (polygon) {
            if (k < 4u || shell_gone) k = 0u;
            if (r == r0) shell_gone = k == 0u;
        }
        ((gw_u32*)c.ring_k)[r] = k | (points ? kSpPoints : 0u);
    }
}

// blockIdx.x: the column; a thread per feature, its gridDim.y * 64 * kSpWaves threads striding over them
__global__ __launch_bounds__(64 * kSpWaves) void simplify_features_kernel(
    const uint8_t* __restrict__ dec, const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb,
    const covt_geom_result* __restrict__ gres, const covt_simplify_desc* __restrict__ sdescs, uint8_t* __restrict__ out,
    const covt_geom_result* __restrict__ ores) {
    const int64_t col = blockIdx.x;
    if (ores[col].status != COVT_OK) return;
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], dec, asmb, out, 0);
    const int l = lane_id();
    const int32_t threads = (int32_t)(gridDim.y * 64 * kSpWaves);
    // (every lane of a wave runs the same number of steps: the wave finishes its wide features together)
    for (int32_t f0 = (int32_t)(blockIdx.y * 64 * kSpWaves + (threadIdx.x & ~63u)); f0 < c.n; f0 += threads) {
        const int32_t f = f0 + l;
        const bool have = f < c.n;
        int32_t g0 = 0, g1 = 0;
        uint32_t t = 0;
        bool wide = false;
        if (have) {
            g0 = c.geo_at(f), g1 = c.geo_at(f + 1);
            t = (uint32_t)((const g_u8*)c.types)[f];
            wide = g1 - g0 >= kSpNarrow || c.part_at(g1) - c.part_at(g0) >= kSpNarrow;
        }
        if (have && !wide)
            for (int32_t g = g0; g < g1; ++g) sp_part(c, g, t);
        // the wide features of this step, one after the other by the whole wave, a lane per part
        for (uint64_t m = __ballot(wide); m; m &= m - 1) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const int32_t wg0 = (int32_t)lane_bcast((uint32_t)g0, src), wg1 = (int32_t)lane_bcast((uint32_t)g1, src);
            const uint32_t wt = lane_bcast(t, src);
            for (int32_t g = wg0 + l; g < wg1; g += 64) sp_part(c, g, wt);
        }
    }
}

// ---- 4. count, 6. write -------------------------------------------------------------------------------
// whether a coordinate that snaps to (x, y) after (bx, by) is kept; r its ring, head: it is the ring's first
__device__ __forceinline__ bool sp_keep(const SpCol& c, int32_t r, bool head, int32_t x, int32_t y, int32_t bx, int32_t by) {
    const uint32_t k = ((g_u32*)c.ring_k)[r];
    return (k & ~kSpPoints) != 0u && ((k & kSpPoints) != 0u || head || x != bx || y != by);
}

// blockIdx.x: the column; a wave per chunk, the column's gridDim.y * kSpWaves waves striding over them.  Per row
// of 128 coordinates the rings that start in it are marked in LDS, a lane per ring (ring + 1 at the start of a
// non-empty ring: one ring per position), and a coordinate's ring is the running maximum of the marks up to it
// (DPP), carried from row to row; the chunk's first by the 64-ary search.
template <bool WRITE>
__global__ __launch_bounds__(64 * kSpWaves) void simplify_stream_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_simplify_desc* __restrict__ sdescs, int32_t shift, const int32_t* __restrict__ d_shift,
    uint8_t* __restrict__ out, const covt_geom_result* __restrict__ ores) {
    __shared__ __attribute__((aligned(16))) uint32_t marks[kSpWaves][128];
    const int64_t col = blockIdx.x;
    if (ores[col].status != COVT_OK) return;
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, sp_shift(shift, d_shift, col));
    const int l = lane_id();
    uint32_t* const mark = marks[threadIdx.x >> 6];
    const int32_t chunks = c.chunks();
    const auto ring_at = [&](int32_t r) { return c.ring_at(r); };
    *(uint64_t*)(mark + 2 * l) = 0ull;
    wave_sync();
    for (int32_t ch = uni((int32_t)(blockIdx.y * kSpWaves + (threadIdx.x >> 6))); ch < chunks;
         ch += (int32_t)(gridDim.y * kSpWaves)) {
        const int32_t A = ch * COVT_SIMPLIFY_CHUNK, B = min(A + COVT_SIMPLIFY_CHUNK, c.V);
        // the ring of the chunk's first coordinate: the last one that starts at or before it
        const int32_t rlo = clamp0(seg_first_at(c.R, A + 1, ring_at) - 1, c.R - 1);
        uint32_t open = (uint32_t)rlo + 1u;  // ring + 1 of the coordinate before the row (uniform)
        int32_t sc = rlo;                    // the first ring not yet marked (uniform; rlo may start at A itself)
        uint32_t run = WRITE ? (uint32_t)uni((int32_t)((g_u32*)c.chunk_k)[ch]) : 0u;
        int32_t px = 0, py = 0;  // the coordinate before the row, snapped (uniform)
        if (A > 0) {
            c.load1(A - 1, px, py);
            px = c.snap(px), py = c.snap(py);
        }
        for (int k = 0; k < kSpRows; ++k) {
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
            const int32_t x0 = c.snap(q.x), y0 = c.snap(q.y), x1 = c.snap(q.z), y1 = c.snap(q.w);
            // the coordinate before this lane's two: the lane before's second (lane 0: the one before the row)
            const int32_t bx = (int32_t)dpp_move<0x138, 0xf>((uint32_t)px, (uint32_t)x1);
            const int32_t by = (int32_t)dpp_move<0x138, 0xf>((uint32_t)py, (uint32_t)y1);
            px = (int32_t)lane_bcast((uint32_t)x1, 63), py = (int32_t)lane_bcast((uint32_t)y1, 63);
            // (r0, r1 are in 1 .. R: open is, and so is every mark)
            const bool k0 = i0 < B && sp_keep(c, (int32_t)r0 - 1, m0 != 0u, x0, y0, bx, by);
            const bool k1 = i0 + 1 < B && sp_keep(c, (int32_t)r1 - 1, m1 != 0u, x1, y1, x0, y0);
            const uint64_t b0 = __ballot(k0), b1 = __ballot(k1);
            if (WRITE) {
                // (a destination is below the column's kept count, itself at most V; checked all the same)
                const uint32_t d0 = run + (uint32_t)(bits_below(b0) + bits_below(b1)), d1 = d0 + (k0 ? 1u : 0u);
                if (k0 && d0 < (uint32_t)c.coord_cap)
                    *(gw_u64*)(c.o_xy + 2 * (int64_t)d0) = (uint64_t)(uint32_t)x0 | ((uint64_t)(uint32_t)y0 << 32);
                if (k1 && d1 < (uint32_t)c.coord_cap)
                    *(gw_u64*)(c.o_xy + 2 * (int64_t)d1) = (uint64_t)(uint32_t)x1 | ((uint64_t)(uint32_t)y1 << 32);
            }
            run += (uint32_t)(__popcll(b0) + __popcll(b1));
            wave_sync();
        }
        if (!WRITE && l == 0) ((gw_u32*)c.chunk_k)[ch] = run;
    }
}

// ---- 5. scan ------------------------------------------------------------------------------------------
// ring_offsets' and num_coords from k'_r, chunk_k -> its exclusive scan in place, the upper two levels copied
template <int NW>
__device__ void simplify_scan_column(const SpCol& c, covt_geom_result* res, AsmSmemT<NW, kSpIpl>& sm) {
    constexpr int K = Coop<NW, kSpIpl>::K;
    const int l = Coop<NW, kSpIpl>::tid();
    auto ioff = [&](int k) { return NW == 1 ? 64 * k + l : kSpIpl * l + k; };
    const uint32_t cap = (uint32_t)c.coord_cap;
    int buf = 0;
    uint32_t base = 0;
    for (int32_t r0 = 0; r0 < c.R; r0 += K) {
        uint32_t x[kSpIpl], ex[kSpIpl], tot;
#pragma unroll
        for (int k = 0; k < kSpIpl; ++k) {
            const int32_t r = r0 + ioff(k);
            x[k] = r < c.R ? ((g_u32*)c.ring_k)[r] & ~kSpPoints : 0u;
        }
        excl_scan4(sm, buf, x, ex, tot);
#pragma unroll
        for (int k = 0; k < kSpIpl; ++k) {
            const int32_t r = r0 + ioff(k);
            if (r < c.R) ((gw_i32*)c.o_ring)[r] = (int32_t)min(add_sat(base, ex[k]), cap);
        }
        base = add_sat(base, tot);
    }
    if (l == 0) {  // (the kept counts of a well-formed column sum to at most V)
        ((gw_i32*)c.o_ring)[c.R] = (int32_t)min(base, cap);
        res->num_coords = (int32_t)min(base, cap);
    }
    const int32_t chunks = c.chunks();
    base = 0;
    for (int32_t h0 = 0; h0 < chunks; h0 += K) {
        uint32_t x[kSpIpl], ex[kSpIpl], tot;
#pragma unroll
        for (int k = 0; k < kSpIpl; ++k) {
            const int32_t h = h0 + ioff(k);
            x[k] = h < chunks ? ((g_u32*)c.chunk_k)[h] : 0u;
        }
        excl_scan4(sm, buf, x, ex, tot);
#pragma unroll
        for (int k = 0; k < kSpIpl; ++k) {
            const int32_t h = h0 + ioff(k);
            if (h < chunks) ((gw_u32*)c.chunk_k)[h] = add_sat(base, ex[k]);
        }
        base = add_sat(base, tot);
    }
    for (int32_t i = l; i <= c.n; i += 64 * NW) ((gw_i32*)c.o_geo)[i] = ((const g_i32*)c.geo)[i];
    for (int32_t i = l; i <= c.P; i += 64 * NW) ((gw_i32*)c.o_part)[i] = ((const g_i32*)c.part)[i];
}

// one wave per column
__global__ __launch_bounds__(64 * kSpWaves) void simplify_scan_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_simplify_desc* __restrict__ sdescs, int64_t n_cols, uint8_t* __restrict__ out,
    covt_geom_result* __restrict__ ores) {
    __shared__ AsmSmemT<1, kSpIpl> smem[kSpWaves];
    const int w = threadIdx.x >> 6;
    const int64_t col = uni64((int64_t)blockIdx.x * kSpWaves + w);
    if (col >= n_cols || ores[col].status != COVT_OK) return;
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, 0);
    simplify_scan_column<1>(c, ores + col, smem[w]);
}

// a workgroup per column (small batches)
__global__ __launch_bounds__(64 * kSpWaves) void simplify_scan_coop_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_simplify_desc* __restrict__ sdescs, int64_t n_cols, uint8_t* __restrict__ out,
    covt_geom_result* __restrict__ ores) {
    __shared__ AsmSmemT<kSpWaves, kSpIpl> smem;
    const int64_t col = blockIdx.x;
    if (col >= n_cols || ores[col].status != COVT_OK) return;  // (uniform over the workgroup)
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, 0);
    simplify_scan_column<kSpWaves>(c, ores + col, smem);
}

}  // namespace covt

extern "C" int covt_geometry_simplify_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                             const covt_geom_result* d_gres, const covt_simplify_desc* d_sdesc,
                                             int64_t n_columns, int32_t shift, const int32_t* d_shift,
                                             uint8_t* d_simplify, covt_geom_result* d_gres_out, void* hip_stream) {
    using namespace covt;
    if (n_columns < 0 || (!d_shift && !simplify_shift_valid(shift)) ||
        (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_sdesc || !d_simplify || !d_gres_out)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || d_asm == d_simplify) return COVT_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)hip_stream;
    const unsigned cols256 = (unsigned)((n_columns + 255) / 256);
    const dim3 grid((unsigned)n_columns, product_blocks_y(n_columns)), block(64 * kSpWaves);
    hipLaunchKernelGGL(simplify_init_kernel, dim3(cols256), dim3(256), 0, s, d_gdesc, d_gres, d_sdesc, n_columns, d_shift,
                       d_gres_out);
    hipLaunchKernelGGL(simplify_rings_kernel, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_sdesc, shift, d_shift, d_simplify,
                       d_gres_out);
    hipLaunchKernelGGL(simplify_features_kernel, grid, block, 0, s, d_decoded, d_gdesc, d_asm, d_gres, d_sdesc, d_simplify,
                       d_gres_out);
    hipLaunchKernelGGL(simplify_stream_kernel<false>, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_sdesc, shift, d_shift,
                       d_simplify, d_gres_out);
    if (n_columns <= kSpCoopMaxColumns)
        hipLaunchKernelGGL(simplify_scan_coop_kernel, dim3((unsigned)n_columns), block, 0, s, d_gdesc, d_asm, d_gres, d_sdesc,
                           n_columns, d_simplify, d_gres_out);
    else
        hipLaunchKernelGGL(simplify_scan_kernel, dim3((unsigned)((n_columns + kSpWaves - 1) / kSpWaves)), block, 0, s,
                           d_gdesc, d_asm, d_gres, d_sdesc, n_columns, d_simplify, d_gres_out);
    hipLaunchKernelGGL(simplify_stream_kernel<true>, grid, block, 0, s, d_gdesc, d_asm, d_gres, d_sdesc, shift, d_shift,
                       d_simplify, d_gres_out);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

// covt_measures.hip -- gfx950 per-feature area, length and vertex counts of assembled geometry columns
// (include/covt.h "Geometry measures"): GeoArrow-style nested offsets + int32 coordinates -> area | length
// float64 and num_coords int32 arrays per column.
//
// A two-level segmented reduction, edges -> rings -> features, in three launches; no allocation, no float
// atomics, every output element and every ring total written exactly once by one thread (so a captured graph
// replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's).
//   2. rings: the column's coordinates are cut into chunks of kMsChunk; every wave of the column's gridDim.y
//      workgroups takes a run of consecutive chunks and owns the rings that start inside its run (an empty
//      ring: where its offset falls; those at the column's end: the last run).  Per chunk a lane loads two
//      coordinates (16 bytes), takes the next one from its neighbour (DPP) and computes the two edge terms to
//      the next coordinate: x_i * y_{i+1} - x_{i+1} * y_i in int64 (mod 2^64) and sqrt(dx * dx + dy * dy) in
//      float64, both zero where the next coordinate starts another ring or the column ends.  Ring heads are
//      marked in LDS by a lane per ring, a segmented inclusive scan keyed on them (DPP, carried from chunk to
//      chunk) goes to LDS, and a lane per ring that ends in the chunk picks the value at its last coordinate
//      up and stores the ring's (S_r, length) in the column's scratch.  The one ring still open at the end of
//      the run is finished by its owner: by the wave if fewer than kMsWide coordinates remain, else by the whole
//      workgroup through LDS once all its waves are through their runs (partial sums added in a fixed order).
//   3. features: a thread per feature.  Its rings are the one range [part[geo[f]], part[geo[f + 1]]), so with
//      A = sum of |S_r| over them and H = sum of |S of the first ring| over its non-empty parts, the shell-
//      minus-holes total is T_f = 2 H - A (mod 2^64, exact).  A feature of fewer than kMsNarrow rings and
//      parts is summed by its thread; the others are finished one after the other by the whole wave, lanes
//      striding over the rings, then a DPP reduction in a fixed order.  The type gate comes from types[],
//      num_coords from start().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_coop.h"
#include "covt_measures_plan.h"
#include "covt_wave.h"

#pragma clang fp contract(off)  // length terms: one rounding per operation, as the header words it

namespace covt {

constexpr int kMsWaves = 4;            // waves per workgroup
constexpr int kMsChunk = 128;          // coordinates per wave chunk: 64 lanes x 2 (one 16-byte load)
constexpr int kMsNarrow = 64;          // rings or parts from which a feature is finished by the whole wave
constexpr int kMsWide = 2048;          // coordinates left past a run from which the workgroup finishes a ring
constexpr int kMsSmallBlocks = 8192;   // workgroups over all columns of a small batch (at most 64 each)
constexpr int kMsMaxBlocksY = 64;

typedef __attribute__((address_space(1))) double gw_f64;
typedef __attribute__((address_space(1))) int64_t gw_i64;
typedef __attribute__((address_space(1))) int32_t gw_i32;
typedef __attribute__((address_space(1))) const int64_t g_i64;
typedef __attribute__((address_space(1))) const double g_f64;

// a partial sum of edge terms: s the doubled signed area mod 2^64, len the length
struct MsSum {
    uint64_t s;
    double len;
};
__device__ __forceinline__ MsSum ms_zero() { return MsSum{0ull, 0.0}; }
__device__ __forceinline__ MsSum ms_add(MsSum a, MsSum b) { return MsSum{a.s + b.s, a.len + b.len}; }
__device__ __forceinline__ MsSum ms_sel(bool p, MsSum a, MsSum b) { return MsSum{p ? a.s : b.s, p ? a.len : b.len}; }
template <int CTRL, int RMASK>
__device__ __forceinline__ uint64_t dpp64(uint64_t old, uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)old, (int)(uint32_t)v, CTRL, RMASK, 0xf, false);
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(old >> 32), (int)(uint32_t)(v >> 32), CTRL, RMASK, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}
// the DPP-moved sum of another lane; lanes without a source read `old`
template <int CTRL, int RMASK>
__device__ __forceinline__ MsSum ms_dpp(MsSum old, MsSum v) {
    MsSum r;
    r.s = dpp64<CTRL, RMASK>(old.s, v.s);
    r.len = __longlong_as_double((long long)dpp64<CTRL, RMASK>((uint64_t)__double_as_longlong(old.len),
                                                               (uint64_t)__double_as_longlong(v.len)));
    return r;
}
// one step of the segmented inclusive scan: (v, f) := (pv, pf) (+) (v, f); a lane with f set starts a segment
// (selects, not branches: the DPP moves run with every lane enabled)
template <int CTRL, int RMASK>
__device__ __forceinline__ void ms_seg_step(MsSum& v, int32_t& f) {
    const MsSum pv = ms_dpp<CTRL, RMASK>(ms_zero(), v);
    const int32_t pf = __builtin_amdgcn_update_dpp(0, f, CTRL, RMASK, 0xf, false);
    v = ms_sel(f != 0, v, ms_add(pv, v));
    f |= pf;
}
template <int CTRL, int RMASK>
__device__ __forceinline__ void ms_red_step(MsSum& v) {
    v = ms_add(ms_dpp<CTRL, RMASK>(ms_zero(), v), v);
}
__device__ __forceinline__ MsSum ms_bcast(MsSum v, int src) {
    return MsSum{lane_bcast64(v.s, src), __longlong_as_double((long long)lane_bcast64((uint64_t)__double_as_longlong(v.len), src))};
}
// the sum of the 64 lanes' values in the fixed order of the wave64 DPP sequence, uniform
__device__ __forceinline__ MsSum ms_wave_sum(MsSum v) {
    ms_red_step<0x111, 0xf>(v);  // row_shr:1
    ms_red_step<0x112, 0xf>(v);  // row_shr:2
    ms_red_step<0x114, 0xf>(v);  // row_shr:4
    ms_red_step<0x118, 0xf>(v);  // row_shr:8
    ms_red_step<0x142, 0xa>(v);  // row_bcast:15
    ms_red_step<0x143, 0xc>(v);  // row_bcast:31
    return ms_bcast(v, 63);
}

// the edge term from (x0, y0) to (x1, y1)
__device__ __forceinline__ MsSum ms_edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    const uint64_t s = (uint64_t)((int64_t)x0 * (int64_t)y1) - (uint64_t)((int64_t)x1 * (int64_t)y0);
    const double dx = (double)x1 - (double)x0, dy = (double)y1 - (double)y0;  // (exact)
    return MsSum{s, sqrt(dx * dx + dy * dy)};
}
__device__ __forceinline__ uint64_t ms_abs(uint64_t s) { return (int64_t)s < 0 ? 0ull - s : s; }

struct MsCol {
    const int32_t *geo, *part, *ring, *xy;
    const uint8_t* types;
    uint8_t* out;  // the column's slice
    int32_t n, P, R, V, ring_cap;
};

__device__ __forceinline__ int32_t ms_clamp(int32_t x, int32_t hi) { return min(max(x, 0), hi); }
// the offsets, indices clamped as the bounding-box pass clamps them: a column whose offsets are not what
// assembly promises is still read inside its slices
__device__ __forceinline__ int32_t ms_geo(const MsCol& c, int32_t f) { return ms_clamp(((const g_i32*)c.geo)[f], c.P); }
__device__ __forceinline__ int32_t ms_part(const MsCol& c, int32_t g) { return ms_clamp(((const g_i32*)c.part)[g], c.R); }
__device__ __forceinline__ int32_t ms_ring(const MsCol& c, int32_t r) { return ms_clamp(((const g_i32*)c.ring)[r], c.V); }

// coordinate i (below V) as (x, y)
__device__ __forceinline__ void ms_load1(const MsCol& c, int32_t i, int32_t& x, int32_t& y) {
    const uint64_t v = *(g_u64*)(c.xy + 2 * (int64_t)i);
    x = (int32_t)(uint32_t)v;
    y = (int32_t)(uint32_t)(v >> 32);
}
// coordinates i, i + 1 (i even: 16-byte aligned) as (x0, y0, x1, y1); those at or past `end` are not read
__device__ __forceinline__ i32x4 ms_load2(const MsCol& c, int32_t i, int32_t end) {
    i32x4 q = i32x4{0, 0, 0, 0};
    if (i + 1 < end) {
        q = *(g_i32x4*)(c.xy + 2 * (int64_t)i);
    } else if (i < end) {
        int32_t x, y;
        ms_load1(c, i, x, y);
        q.x = x, q.y = y;
    }
    return q;
}

// the first ring r in [0, R] with ring(r) >= x (ring nondecreasing): the wave probes 64 evenly spaced rings
// per step (x uniform)
__device__ __forceinline__ int32_t ms_first_at(const MsCol& c, int32_t x) {
    int32_t lo = 0, hi = c.R;
    while (lo < hi) {
        const int32_t step = (hi - lo + 63) >> 6;
        const int32_t p = min(lo + lane_id() * step, hi);
        const bool below = p < hi && ms_ring(c, p) < x;  // (a prefix of the lanes)
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

struct __attribute__((aligned(16))) MsSmem {
    uint64_t res_s[kMsWaves][kMsChunk];     // the chunk's inclusive segmented sums per coordinate
    double res_len[kMsWaves][kMsChunk];
    uint8_t head[kMsWaves][kMsChunk + 4];   // 1: a ring starts at this coordinate of the chunk (0 .. kMsChunk)
    uint64_t wide_s[kMsWaves];              // a wave's ring left to the workgroup: its sums so far,
    double wide_len[kMsWaves];
    int32_t wide_r[kMsWaves];               //   its index (-1: none),
    int32_t wide_from[kMsWaves];            //   and the coordinates [from, to) whose edges are still to take
    int32_t wide_to[kMsWaves];
    uint64_t red_s[kMsWaves];
    double red_len[kMsWaves];
};

__device__ __forceinline__ void ms_column(const covt_geom_desc& gd, const covt_geom_result& gr, const covt_measures_desc& md,
                                          const uint8_t* dec, const uint8_t* asmb, uint8_t* out, MsCol& c) {
    c.geo = (const int32_t*)(asmb + gd.out_off[0]);
    c.part = (const int32_t*)(asmb + gd.out_off[1]);
    c.ring = (const int32_t*)(asmb + gd.out_off[2]);
    c.xy = (const int32_t*)(asmb + gd.out_off[3]);
    c.types = dec ? dec + gd.in_off[0] : nullptr;  // (the rings kernel reads no types)
    c.out = out + md.off;
    c.n = md.n_features;
    c.ring_cap = md.ring_cap;
    c.P = ms_clamp(gr.num_parts, gd.part_cap);
    c.R = ms_clamp(gr.num_rings, gd.ring_cap);
    c.V = ms_clamp(gr.num_coords, gd.coord_cap);
}
__device__ __forceinline__ void ms_put_ring(const MsCol& c, int32_t r, MsSum v) {
    ((gw_i64*)(c.out + measures_ring_s_off(c.n, c.ring_cap)))[r] = (int64_t)v.s;
    ((gw_f64*)(c.out + measures_ring_len_off(c.n, c.ring_cap)))[r] = v.len;
}

// the column's status before any work: the assembly's, then the layout's
__device__ __forceinline__ int32_t measures_precheck(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                     const covt_measures_desc& md) {
    if (gr.status != COVT_OK) return gr.status;
    if (((uint32_t)gd.flags & COVT_GEOM_TOO_LARGE) || (md.flags & COVT_MEASURES_TOO_LARGE) || md.off < 0 || (md.off & 15))
        return COVT_ERR_INVALID_ARG;
    const int32_t n = gd.in_off[0] >= 0 ? gd.in_len[0] : 0;  // the features the assembly walked
    return md.n_features == n && md.ring_cap == gd.ring_cap ? COVT_OK : COVT_ERR_INVALID_ARG;
}

// ---- 1. init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void measures_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                            const covt_geom_result* __restrict__ gres,
                                                            const covt_measures_desc* __restrict__ mdescs,
                                                            int64_t n_cols, covt_measures_result* __restrict__ mres) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    int32_t* r = (int32_t*)(mres + c);
    r[0] = measures_precheck(gdescs[c], gres[c], mdescs[c]);
    r[1] = 0;
}

// ---- 2. rings -----------------------------------------------------------------------------------------
// blockIdx.x: the column; each of its gridDim.y * kMsWaves waves takes a run of consecutive chunks
__global__ __launch_bounds__(64 * kMsWaves) void measures_rings_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                                       const uint8_t* __restrict__ asmb,
                                                                       const covt_geom_result* __restrict__ gres,
                                                                       const covt_measures_desc* __restrict__ mdescs,
                                                                       uint8_t* __restrict__ out,
                                                                       const covt_measures_result* __restrict__ mres) {
    __shared__ MsSmem sm;
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    MsCol c;
    ms_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out, c);
    const int l = lane_id();
    const int w = threadIdx.x >> 6;
    const int32_t wave = uni((int32_t)(blockIdx.y * kMsWaves + w));
    const int32_t waves = (int32_t)(gridDim.y * kMsWaves);
    // (a column without coordinates is one chunk of none: its rings are all empty)
    const int64_t chunks = std::max<int64_t>(1, ((int64_t)c.V + kMsChunk - 1) / kMsChunk);
    const int32_t cb = (int32_t)(chunks * wave / waves), ce = (int32_t)(chunks * (wave + 1) / waves);
    int32_t wide_r = -1, wide_from = 0, wide_to = 0;
    MsSum carry = ms_zero();
    auto run = [&]() {  // the wave's run (uniform over the wave; the workgroup's barriers come after it)
    if (cb >= ce || c.R <= 0) return;
    uint64_t* const res_s = sm.res_s[w];
    double* const res_len = sm.res_len[w];
    uint8_t* const head = sm.head[w];

    const bool last = ce == chunks;  // the column's last run: owns the empty rings at its end
    const int32_t A = cb * kMsChunk, B = last ? c.V : ce * kMsChunk;
    int32_t rc = A == 0 ? 0 : ms_first_at(c, A);  // the first ring not yet stored
    for (int l4 = 4 * l; l4 < kMsChunk + 4; l4 += 256) *(uint32_t*)(head + l4) = 0;
    wave_sync();
    for (int32_t j = cb; j < ce && rc < c.R; ++j) {
        const int32_t a = j * kMsChunk, L = min(kMsChunk, c.V - a), b = a + L;
        const int32_t s_rc = uni(ms_ring(c, rc));
        if (!last && s_rc >= B) break;  // the next ring starts in a later run
        const bool process = s_rc < b;  // a ring of this wave's has a coordinate here
        if (!process && j != chunks - 1) continue;
        if (process) {
            const int32_t p0 = 2 * l;
            const i32x4 q = ms_load2(c, a + p0, b);
            int32_t tx = 0, ty = 0;  // the coordinate after the chunk (uniform)
            if (b < c.V) ms_load1(c, b, tx, ty);
            // heads: the rings from rc on that start at or below b (ring R: the column's end)
            for (int32_t rh = rc;; rh += 64) {
                const int32_t r = rh + l;
                const int32_t s = r <= c.R ? ms_ring(c, r) : 0x7fffffff;
                const bool in = r <= c.R && s <= b;
                if (in && (uint32_t)(s - a) <= (uint32_t)L) head[s - a] = 1;
                if (__ballot(in) != ~0ull) break;
            }
            wave_sync();
            const uint32_t hh = *(const uint16_t*)(head + p0);
            const int32_t h0 = (int32_t)(hh & 0xffu), h1 = (int32_t)(hh >> 8);
            const int32_t h2 = head[p0 + 2];
            // the coordinate after this lane's two: the next lane's first (lane 63: the one after the chunk)
            const int32_t nx = (int32_t)lane_next((uint32_t)q.x, (uint32_t)tx);
            const int32_t ny = (int32_t)lane_next((uint32_t)q.y, (uint32_t)ty);
            const MsSum e0 = ms_edge(q.x, q.y, q.z, q.w), e1 = ms_edge(q.z, q.w, nx, ny);
            const MsSum t0 = ms_sel(a + p0 + 1 < c.V && h1 == 0 && p0 + 1 < L, e0, ms_zero());
            const MsSum t1 = ms_sel(a + p0 + 2 < c.V && h2 == 0 && p0 + 1 < L, e1, ms_zero());
            // the segmented inclusive scan over the chunk, carried in from the chunk before
            MsSum v = ms_sel(h1 != 0, t1, ms_add(t0, t1));
            int32_t f = h0 | h1;
            v = ms_sel(l == 0 && f == 0, ms_add(carry, v), v);
            ms_seg_step<0x111, 0xf>(v, f);  // row_shr:1
            ms_seg_step<0x112, 0xf>(v, f);  // row_shr:2
            ms_seg_step<0x114, 0xf>(v, f);  // row_shr:4
            ms_seg_step<0x118, 0xf>(v, f);  // row_shr:8
            ms_seg_step<0x142, 0xa>(v, f);  // row_bcast:15
            ms_seg_step<0x143, 0xc>(v, f);  // row_bcast:31
            const MsSum ex = ms_dpp<0x138, 0xf>(carry, v);  // wave_shr:1: the lane before (lane 0: the carry)
            const MsSum r0 = ms_sel(h0 != 0, t0, ms_add(ex, t0));
            const MsSum r1 = ms_sel(h1 != 0, t1, ms_add(r0, t1));
            carry = ms_bcast(v, 63);
            res_s[p0] = r0.s, res_s[p0 + 1] = r1.s;
            res_len[p0] = r0.len, res_len[p0 + 1] = r1.len;
            wave_sync();
            for (int l4 = 4 * l; l4 < kMsChunk + 4; l4 += 256) *(uint32_t*)(head + l4) = 0;  // (read above)
        }
        // the rings that end in this chunk: a lane each, in steps of 64
        for (;;) {
            const int32_t r = rc + l;
            const int32_t s = r < c.R ? ms_ring(c, r) : 0, e = r < c.R ? ms_ring(c, r + 1) : 0;
            const bool done = r < c.R && (last || s < B) && e <= b;  // (a prefix of the lanes)
            if (done) {
                const uint32_t at = (uint32_t)(e - 1 - a);
                const bool any = e > s && process && at < (uint32_t)kMsChunk;
                ms_put_ring(c, r, any ? MsSum{res_s[at], res_len[at]} : ms_zero());
            }
            const int cnt = __popcll(__ballot(done));
            rc += cnt;
            if (cnt < 64) break;
        }
        wave_sync();  // (res and head are rewritten by the next chunk)
    }
    // the ring still open at the end of the run: the edges from the coordinates [B, e - 1) are left
    if (!last && rc < c.R) {
        const int32_t s = uni(ms_ring(c, rc)), e = uni(ms_ring(c, rc + 1));
        if (s < B && e > B && e - B >= kMsWide) {
            wide_r = rc, wide_from = B, wide_to = e;
        } else if (s < B && e > B) {
            MsSum part = ms_zero();
            for (int32_t i = B + l; i + 1 < e; i += 64) {
                int32_t x0, y0, x1, y1;
                ms_load1(c, i, x0, y0);
                ms_load1(c, i + 1, x1, y1);
                part = ms_add(part, ms_edge(x0, y0, x1, y1));
            }
            const MsSum tot = ms_add(carry, ms_wave_sum(part));
            if (l == 0) ms_put_ring(c, rc, tot);
        }
    }
    };
    run();
    if (l == 0) {
        sm.wide_r[w] = wide_r;
        sm.wide_from[w] = wide_from;
        sm.wide_to[w] = wide_to;
        sm.wide_s[w] = carry.s;
        sm.wide_len[w] = carry.len;
    }
    __syncthreads();
    // rings left to the workgroup: all its threads take the remaining edges, then the waves' sums in wave order
    for (int k = 0; k < kMsWaves; ++k) {
        const int32_t r = sm.wide_r[k];
        if (r < 0) continue;  // (uniform)
        const int32_t from = sm.wide_from[k], to = sm.wide_to[k];
        MsSum part = ms_zero();
        for (int32_t i = from + (int32_t)threadIdx.x; i + 1 < to; i += 64 * kMsWaves) {
            int32_t x0, y0, x1, y1;
            ms_load1(c, i, x0, y0);
            ms_load1(c, i + 1, x1, y1);
            part = ms_add(part, ms_edge(x0, y0, x1, y1));
        }
        part = ms_wave_sum(part);
        if (l == 0) sm.red_s[w] = part.s, sm.red_len[w] = part.len;
        __syncthreads();
        if (threadIdx.x == 0) {
            MsSum tot = MsSum{sm.wide_s[k], sm.wide_len[k]};
#pragma unroll
            for (int i = 0; i < kMsWaves; ++i) tot = ms_add(tot, MsSum{sm.red_s[i], sm.red_len[i]});
            ms_put_ring(c, r, tot);
        }
        __syncthreads();
    }
}

// ---- 3. features --------------------------------------------------------------------------------------
// blockIdx.x: the column; a thread per feature, its gridDim.y * 64 * kMsWaves threads striding over them
__global__ __launch_bounds__(64 * kMsWaves) void measures_features_kernel(const uint8_t* __restrict__ dec,
                                                                          const covt_geom_desc* __restrict__ gdescs,
                                                                          const uint8_t* __restrict__ asmb,
                                                                          const covt_geom_result* __restrict__ gres,
                                                                          const covt_measures_desc* __restrict__ mdescs,
                                                                          uint8_t* __restrict__ out,
                                                                          const covt_measures_result* __restrict__ mres) {
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;
    MsCol c;
    ms_column(gdescs[col], gres[col], mdescs[col], dec, asmb, out, c);
    const g_i64* const ring_s = (const g_i64*)(c.out + measures_ring_s_off(c.n, c.ring_cap));
    const g_f64* const ring_len = (const g_f64*)(c.out + measures_ring_len_off(c.n, c.ring_cap));
    gw_f64* const o_area = (gw_f64*)(c.out + measures_area_off(c.n));
    gw_f64* const o_len = (gw_f64*)(c.out + measures_length_off(c.n));
    gw_i32* const o_cnt = (gw_i32*)(c.out + measures_count_off(c.n));
    const int l = lane_id();
    const int32_t threads = (int32_t)(gridDim.y * 64 * kMsWaves);
    // (every lane of a wave runs the same number of steps: the wave finishes its wide features together)
    for (int32_t f0 = (int32_t)(blockIdx.y * 64 * kMsWaves + (threadIdx.x & ~63u)); f0 < c.n; f0 += threads) {
        const int32_t f = f0 + l;
        const bool have = f < c.n;
        int32_t g0 = 0, g1 = 0, r0 = 0, r1 = 0;
        uint32_t t = 0;
        if (have) {
            g0 = ms_geo(c, f), g1 = ms_geo(c, f + 1);
            r0 = ms_part(c, g0), r1 = ms_part(c, g1);
            t = (uint32_t)((const g_u8*)c.types)[f];
            o_cnt[f] = ms_ring(c, r1) - ms_ring(c, r0);
        }
        const bool polygon = t == 2u || t == 5u, line = polygon || t == 1u || t == 4u;
        const bool wide = have && line && (r1 - r0 >= kMsNarrow || g1 - g0 >= kMsNarrow);
        if (have && !wide) {
            uint64_t all = 0, shells = 0;
            double len = 0.0;
            if (line)
                for (int32_t r = r0; r < r1; ++r) {
                    all += ms_abs((uint64_t)ring_s[r]);
                    len += ring_len[r];
                }
            if (polygon)
                for (int32_t g = g0; g < g1; ++g) {
                    const int32_t pr = ms_part(c, g);
                    if (ms_part(c, g + 1) > pr && pr < c.R) shells += ms_abs((uint64_t)ring_s[pr]);
                }
            o_area[f] = polygon ? (double)(int64_t)(2 * shells - all) * 0.5 : 0.0;
            o_len[f] = len;
        }
        // the wide features of this step, one after the other by the whole wave
        for (uint64_t m = __ballot(wide); m; m &= m - 1) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const int32_t wf = f0 + src;
            const int32_t wg0 = (int32_t)lane_bcast((uint32_t)g0, src), wg1 = (int32_t)lane_bcast((uint32_t)g1, src);
            const int32_t wr0 = (int32_t)lane_bcast((uint32_t)r0, src), wr1 = (int32_t)lane_bcast((uint32_t)r1, src);
            const bool wpoly = lane_bcast(polygon ? 1u : 0u, src) != 0u;
            MsSum all = ms_zero();
            uint64_t shells = 0;
            for (int32_t r = wr0 + l; r < wr1; r += 64) all = ms_add(all, MsSum{ms_abs((uint64_t)ring_s[r]), ring_len[r]});
            if (wpoly)
                for (int32_t g = wg0 + l; g < wg1; g += 64) {
                    const int32_t pr = ms_part(c, g);
                    if (ms_part(c, g + 1) > pr && pr < c.R) shells += ms_abs((uint64_t)ring_s[pr]);
                }
            all = ms_wave_sum(all);
            shells = lane_bcast64(incl_scan64(shells), 63);
            if (l == 0) {
                o_area[wf] = wpoly ? (double)(int64_t)(2 * shells - all.s) * 0.5 : 0.0;
                o_len[wf] = all.len;
            }
        }
    }
}

}  // namespace covt

extern "C" int covt_geometry_measures_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                             const covt_geom_result* d_gres, const covt_measures_desc* d_mdesc,
                                             int64_t n_columns, uint8_t* d_measures, covt_measures_result* d_mres,
                                             void* hip_stream) {
    using namespace covt;
    if (n_columns < 0 ||
        (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_mdesc || !d_measures || !d_mres)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff) return COVT_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)hip_stream;
    const unsigned cols256 = (unsigned)((n_columns + 255) / 256);
    hipLaunchKernelGGL(measures_init_kernel, dim3(cols256), dim3(256), 0, s, d_gdesc, d_gres, d_mdesc, n_columns, d_mres);
    // small batches: up to 64 workgroups per column, as the bounding-box pass sizes them
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(kMsMaxBlocksY, kMsSmallBlocks / n_columns));
    const dim3 grid((unsigned)n_columns, (unsigned)gy);
    hipLaunchKernelGGL(measures_rings_kernel, grid, dim3(64 * kMsWaves), 0, s, d_gdesc, d_asm, d_gres, d_mdesc, d_measures,
                       d_mres);
    hipLaunchKernelGGL(measures_features_kernel, grid, dim3(64 * kMsWaves), 0, s, d_decoded, d_gdesc, d_asm, d_gres, d_mdesc,
                       d_measures, d_mres);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

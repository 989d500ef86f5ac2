// covt_measures.hip -- gfx950 per-feature area, length and vertex counts of assembled geometry columns
// (include/covt.h "Geometry measures"): GeoArrow-style nested offsets + int32 coordinates -> area | length
// float64 and num_coords int32 arrays per column.
//
// A two-level segmented reduction, edges -> rings -> features, in three launches; no allocation, no float
// atomics, every output element and every ring total written exactly once by one thread (so a captured graph
// replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's).
//   2. rings: the segmented reduction of covt_segscan.h (the chunks, the runs and their owners, the hand-over
//      to the workgroup: described there) under RingPolicy: the segments are the rings, read from ring[]
//      directly, the value is (S, length) under addition, a chunk is one row of 128 coordinates (16 bytes a
//      lane), and a coordinate's term is its edge to the next one -- the lane takes it from its neighbour (DPP)
//      -- x_i * y_{i+1} - x_{i+1} * y_i in int64 (mod 2^64) and sqrt(dx * dx + dy * dy) in float64, both zero
//      where the next coordinate starts another ring or the column ends (so heads are marked up to and
//      including the chunk's end).  A ring's (S_r, length) goes to the column's scratch; the workgroup's
//      partial sums are added in a fixed order.
//   3. features: a thread per feature.  Its rings are the one range [part[geo[f]], part[geo[f + 1]]), so with
//      A = sum of |S_r| over them and H = sum of |S of the first ring| over its non-empty parts, the shell-
//      minus-holes total is T_f = 2 H - A (mod 2^64, exact).  A feature of fewer than kMsNarrow rings and
//      parts is summed by its thread; the others are finished one after the other by the whole wave, lanes
//      striding over the rings, then a DPP reduction in a fixed order.  The type gate comes from types[],
//      num_coords from start().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt.h"
#include "covt_measures_plan.h"
#include "covt_segscan.h"

#pragma clang fp contract(off)  // length terms: one rounding per operation, as the header words it

namespace covt {

constexpr int kMsWaves = 4;    // waves per workgroup
constexpr int kMsNarrow = 64;  // rings or parts from which a feature is finished by the whole wave

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
struct SumV {
    typedef MsSum T;
    static __device__ __forceinline__ T id() { return T{0ull, 0.0}; }
    static __device__ __forceinline__ T join(T a, T b) { return T{a.s + b.s, a.len + b.len}; }
    static __device__ __forceinline__ T sel(bool p, T a, T b) { return T{p ? a.s : b.s, p ? a.len : b.len}; }
    static __device__ __forceinline__ uint64_t bits(double x) { return (uint64_t)__double_as_longlong(x); }
    static __device__ __forceinline__ double f64(uint64_t x) { return __longlong_as_double((long long)x); }
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ T dpp(T old, T v) {
        return T{dpp_move<CTRL, RMASK>(old.s, v.s), f64(dpp_move<CTRL, RMASK>(bits(old.len), bits(v.len)))};
    }
    static __device__ __forceinline__ T bcast(T v, int src) {
        return T{lane_bcast64(v.s, src), f64(lane_bcast64(bits(v.len), src))};
    }
    // (two arrays, not an array of structs: a lane's 16 bytes of either stay one LDS access)
    template <int N>
    struct Lds {
        uint64_t s[N];
        double len[N];
        __device__ __forceinline__ T get(int i) const { return T{s[i], len[i]}; }
        __device__ __forceinline__ void put(int i, T v) { s[i] = v.s, len[i] = v.len; }
    };
};

// the edge term from (x0, y0) to (x1, y1)
__device__ __forceinline__ MsSum ms_edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    const uint64_t s = shoelace_term(x0, y0, x1, y1);
    const double dx = (double)x1 - (double)x0, dy = (double)y1 - (double)y0;  // (exact)
    return MsSum{s, sqrt(dx * dx + dy * dy)};
}
__device__ __forceinline__ uint64_t ms_abs(uint64_t s) { return (int64_t)s < 0 ? 0ull - s : s; }

struct MsCol : GeomCol {
    const uint8_t* types;
    uint8_t* out;  // the column's slice
    int32_t ring_cap;
};
__device__ __forceinline__ MsCol ms_column(const covt_geom_desc& gd, const covt_geom_result& gr, const covt_measures_desc& md,
                                           const uint8_t* dec, const uint8_t* asmb, uint8_t* out) {
    MsCol c;
    (GeomCol&)c = geom_col(gd, gr, asmb, md.n_features);
    c.types = dec ? dec + gd.in_off[0] : nullptr;  // (the rings kernel reads no types)
    c.out = out + md.off;
    c.ring_cap = md.ring_cap;
    return c;
}

// The rings of a column as the segments of covt_segscan.h.
struct RingPolicy {
    typedef SumV V;
    static constexpr int kWaves = kMsWaves;
    static constexpr int kRows = 1;     // one row of 64 lanes x 2 coordinates per chunk: 128 coordinates
    static constexpr int kWide = 2048;  // coordinates left past a run from which the workgroup finishes a ring
    static constexpr int kIncl = 1;     // an edge's term depends on whether the next coordinate is a head
    static constexpr int kAhead = 1;
    struct Raw {
        i32x4 q;
        int32_t tx, ty;  // the coordinate after the chunk (uniform)
    };

    const MsCol& c;

    __device__ __forceinline__ int32_t count() const { return c.R; }
    __device__ __forceinline__ int32_t items() const { return c.V; }
    __device__ __forceinline__ int32_t first_at(int32_t x) const {
        return seg_first_at(c.R, x, [&](int32_t r) { return c.ring_at(r); });
    }
    __device__ __forceinline__ void open(int32_t) {}
    __device__ __forceinline__ void ensure(int32_t, int32_t) {}
    __device__ __forceinline__ int32_t start(int32_t r) const { return r <= c.R ? c.ring_at(r) : 0x7fffffff; }
    __device__ __forceinline__ void load(Raw& r, int32_t a, int32_t b) const {
        r.q = c.load2(a + 2 * lane_id(), b);
        r.tx = r.ty = 0;
        if (b < c.V) c.load1(b, r.tx, r.ty);
    }
    __device__ __forceinline__ void terms(const Raw& r, int, int32_t a, int32_t p0, int32_t L, int32_t h1, int32_t h2,
                                          MsSum& t0, MsSum& t1) const {
        // the coordinate after this lane's two: the next lane's first (lane 63: the one after the chunk)
        const int32_t nx = (int32_t)lane_next((uint32_t)r.q.x, (uint32_t)r.tx);
        const int32_t ny = (int32_t)lane_next((uint32_t)r.q.y, (uint32_t)r.ty);
        const MsSum e0 = ms_edge(r.q.x, r.q.y, r.q.z, r.q.w), e1 = ms_edge(r.q.z, r.q.w, nx, ny);
        t0 = V::sel(a + p0 + 1 < c.V && h1 == 0 && p0 + 1 < L, e0, V::id());
        t1 = V::sel(a + p0 + 2 < c.V && h2 == 0 && p0 + 1 < L, e1, V::id());
    }
    // the edges from the coordinates [from, to - 1)
    __device__ __forceinline__ MsSum tail(int32_t from, int32_t to, int32_t tid, int32_t threads) const {
        MsSum part = V::id();
        for (int32_t i = from + tid; i + 1 < to; i += threads) {
            int32_t x0, y0, x1, y1;
            c.load1(i, x0, y0);
            c.load1(i + 1, x1, y1);
            part = V::join(part, ms_edge(x0, y0, x1, y1));
        }
        return part;
    }
    __device__ __forceinline__ void put(int32_t r, MsSum v, bool) const {
        ((gw_i64*)(c.out + measures_ring_s_off(c.n, c.ring_cap)))[r] = (int64_t)v.s;
        ((gw_f64*)(c.out + measures_ring_len_off(c.n, c.ring_cap)))[r] = v.len;
    }
};

// ---- 1. init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void measures_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                            const covt_geom_result* __restrict__ gres,
                                                            const covt_measures_desc* __restrict__ mdescs,
                                                            int64_t n_cols, covt_measures_result* __restrict__ mres) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    int32_t* r = (int32_t*)(mres + c);
    const covt_measures_desc md = mdescs[c];
    int32_t st = geom_product_precheck(gdescs[c], gres[c], (md.flags & COVT_MEASURES_TOO_LARGE) != 0,
                                       md.off >= 0 && !(md.off & 15), md.n_features);
    if (st == COVT_OK && md.ring_cap != gdescs[c].ring_cap) st = COVT_ERR_INVALID_ARG;
    r[0] = st;
    r[1] = 0;
}

// ---- 2. rings -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kMsWaves) void measures_rings_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_measures_desc* __restrict__ mdescs, uint8_t* __restrict__ out,
    const covt_measures_result* __restrict__ mres) {
    __shared__ SegSmem<RingPolicy> sm;
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const MsCol c = ms_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out);
    RingPolicy p{c};
    seg_run(p, sm);
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
    const MsCol c = ms_column(gdescs[col], gres[col], mdescs[col], dec, asmb, out);
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
            g0 = c.geo_at(f), g1 = c.geo_at(f + 1);
            r0 = c.part_at(g0), r1 = c.part_at(g1);
            t = (uint32_t)((const g_u8*)c.types)[f];
            o_cnt[f] = c.ring_at(r1) - c.ring_at(r0);
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
                    const int32_t pr = c.part_at(g);
                    if (c.part_at(g + 1) > pr && pr < c.R) shells += ms_abs((uint64_t)ring_s[pr]);
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
            MsSum all = SumV::id();
            uint64_t shells = 0;
            for (int32_t r = wr0 + l; r < wr1; r += 64) all = SumV::join(all, MsSum{ms_abs((uint64_t)ring_s[r]), ring_len[r]});
            if (wpoly)
                for (int32_t g = wg0 + l; g < wg1; g += 64) {
                    const int32_t pr = c.part_at(g);
                    if (c.part_at(g + 1) > pr && pr < c.R) shells += ms_abs((uint64_t)ring_s[pr]);
                }
            all = seg_wave_join<SumV>(all);
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
    const dim3 grid((unsigned)n_columns, product_blocks_y(n_columns));
    hipLaunchKernelGGL(measures_rings_kernel, grid, dim3(64 * kMsWaves), 0, s, d_gdesc, d_asm, d_gres, d_mdesc, d_measures,
                       d_mres);
    hipLaunchKernelGGL(measures_features_kernel, grid, dim3(64 * kMsWaves), 0, s, d_decoded, d_gdesc, d_asm, d_gres, d_mdesc,
                       d_measures, d_mres);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

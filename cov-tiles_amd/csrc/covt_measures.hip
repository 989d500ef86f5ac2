// covt_measures.hip -- gfx950 per-feature area, length and vertex counts of assembled geometry columns
// (include/covt.h "Geometry measures"): GeoArrow-style nested offsets + int32 coordinates -> area | length
// float64 and num_coords int32 arrays per column.
//
// A two-level segmented reduction, edges -> rings -> features, in three launches; no allocation, no float
// atomics, every output element and every ring total written exactly once by one thread (so a captured graph
// replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's).
//   2. rings: the segmented reduction of covt_segscan.h over the rings' edges (seg_run under RingEdgePolicy:
//      the chunks, the runs and their owners, the hand-over to the workgroup and the edge's neighbour fetch
//      are described there).  The value is (S, length) under addition and an edge's term (MsEdge)
//      x_i * y_{i+1} - x_{i+1} * y_i in int64 (mod 2^64) and sqrt(dx * dx + dy * dy) in float64.  A ring's
//      (S_r, length) goes to the column's scratch; the partial sums are added in a fixed order.
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

// what the rings pass supplies to RingEdgePolicy: the coordinates as they are, ms_edge, a ring's two sums
struct MsEdge {
    typedef SumV V;
    const MsCol& c;
    __device__ __forceinline__ int32_t map(int32_t v) const { return v; }
    __device__ __forceinline__ MsSum edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) const {
        return ms_edge(x0, y0, x1, y1);
    }
    __device__ __forceinline__ void put(int32_t r, MsSum v, bool) const {
        ((gw_i64*)(c.out + measures_ring_s_off(c.n, c.ring_cap)))[r] = (int64_t)v.s;
        ((gw_f64*)(c.out + measures_ring_len_off(c.n, c.ring_cap)))[r] = v.len;
    }
};
typedef RingEdgePolicy<MsEdge, kMsWaves> MsRings;

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
    __shared__ SegSmem<MsRings> sm;
    const int64_t col = blockIdx.x;
    if (mres[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const MsCol c = ms_column(gdescs[col], gres[col], mdescs[col], nullptr, asmb, out);
    const MsEdge e{c};
    MsRings p{c, e};
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
        wave_each(wide, [&](int src) {
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
        });
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

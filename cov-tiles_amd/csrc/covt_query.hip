// covt_query.hip -- gfx950 exact window and point queries over assembled geometry columns (include/covt.h
// "Geometry queries"): per feature, INTERSECTS or WITHIN a closed int32 window, from the coordinates, written
// into the keep masks of the select buffer (or ANDed into them).  The rules are covt_query_plan.h's; this file is
// the launch and the memory shape, that of covt_measures.hip.
//
// A two-level segmented reduction, edges -> rings -> features, no allocation, no atomics, every ring byte and
// every mask byte written exactly once by one thread (so a captured graph replays the pass as it is):
//
//   1. init (only with a status array): the column's status, query_col_status, to d_status.  The two kernels
//      below compute the same status from the same descriptors; there is no result record to hand it on in.
//   2. rings: the segmented reduction of covt_segscan.h over the rings' edges (seg_run under RingEdgePolicy).
//      The value is one dword of three bits, touch | out << 1 | par << 2, under query_join (OR, OR, XOR), an
//      edge's term query_edge.  A ring's byte goes to the column's scratch, the first ring_cap bytes of the
//      select slice's `bytes` member (the select pass writes that member afterwards).  A ring of exactly one
//      coordinate has no edge, so the thread that puts it loads the coordinate and tests in().
//   3. features: a thread per feature joins its rings' bytes (the one range [part[geo[f]], part[geo[f + 1]])),
//      a feature of kQyNarrow rings or more is finished by the whole wave, lanes striding over the rings, then
//      a DPP reduction.  With types[] and whether the feature has a coordinate that is P_f (query_feature); the
//      thread stores mask[f] (WRITE) or reads, combines and stores it (AND).  A column with a status gets its
//      mask zeroed here.
//
// The window and the two switches travel as one by-value kernel argument of six scalars (QueryArgs), never
// indexed at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt.h"
#include "covt_query_plan.h"
#include "covt_segscan.h"
#include "covt_select_plan.h"

namespace covt {

constexpr int kQyWaves = 4;    // waves per workgroup
constexpr int kQyNarrow = 64;  // rings from which a feature is finished by the whole wave

struct QueryArgs {
    QueryWindow w;
    int32_t relation, mode;
};

// a ring's three bits under query_join
struct QueryV {
    typedef uint32_t T;
    static __device__ __forceinline__ T id() { return 0u; }
    static __device__ __forceinline__ T join(T a, T b) { return query_join(a, b); }
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

// the column's status before any work: the other products' precheck, then the scratch's room
__device__ __forceinline__ int32_t query_col_status(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                    const covt_select_desc& sd) {
    const int32_t st = geom_product_precheck(gd, gr, (sd.flags & COVT_SELECT_TOO_LARGE) != 0,
                                             sd.off >= 0 && !(sd.off & 15), sd.n_features);
    if (st == COVT_OK && sd.byte_cap < (int64_t)gd.ring_cap) return COVT_ERR_INVALID_ARG;
    return st;
}

struct QueryCol : GeomCol {
    const uint8_t* types;
    uint8_t* mask;
    uint8_t* ring_bits;  // the scratch: a byte per ring
};
__device__ __forceinline__ QueryCol query_column(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                 const covt_select_desc& sd, const uint8_t* dec, const uint8_t* asmb,
                                                 uint8_t* select) {
    QueryCol c;
    (GeomCol&)c = geom_col(gd, gr, asmb, sd.n_features);
    c.types = dec ? dec + gd.in_off[0] : nullptr;  // (the rings kernel reads no types)
    c.mask = select + sd.off + select_mask_off(sd.n_features);
    c.ring_bits = select + sd.off + select_bytes_off(sd.n_features);
    return c;
}

// what the rings pass supplies to RingEdgePolicy: the coordinates as they are, query_edge, a ring's byte
struct QueryEdge {
    typedef QueryV V;
    const QueryCol& c;
    const QueryWindow w;
    __device__ __forceinline__ int32_t map(int32_t v) const { return v; }
    __device__ __forceinline__ uint32_t edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) const {
        return query_edge(w, x0, y0, x1, y1);
    }
    __device__ __forceinline__ void put(int32_t r, uint32_t v, bool any) const {
        if (any) {
            const int32_t a = c.ring_at(r);
            if (c.ring_at(r + 1) - a == 1) {  // (no edge has seen this coordinate)
                int32_t x, y;
                c.load1(a, x, y);
                v = query_point(w, x, y);
            }
        }
        ((gw_u8*)c.ring_bits)[r] = (uint8_t)v;
    }
};
typedef RingEdgePolicy<QueryEdge, kQyWaves> QueryRings;

// ---- 1. init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void query_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                         const covt_geom_result* __restrict__ gres,
                                                         const covt_select_desc* __restrict__ sdescs, int64_t n_cols,
                                                         int32_t* __restrict__ status) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    status[c] = query_col_status(gdescs[c], gres[c], sdescs[c]);
}

// ---- 2. rings -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kQyWaves) void query_rings_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                                    const uint8_t* __restrict__ asmb,
                                                                    const covt_geom_result* __restrict__ gres,
                                                                    const covt_select_desc* __restrict__ sdescs,
                                                                    uint8_t* __restrict__ select, QueryArgs q) {
    __shared__ SegSmem<QueryRings> sm;
    const int64_t col = blockIdx.x;
    const covt_geom_desc gd = gdescs[col];
    const covt_geom_result gr = gres[col];
    const covt_select_desc sd = sdescs[col];
    if (query_col_status(gd, gr, sd) != COVT_OK) return;  // (uniform over the workgroup)
    const QueryCol c = query_column(gd, gr, sd, nullptr, asmb, select);
    const QueryEdge e{c, q.w};
    QueryRings p{c, e};
    seg_run(p, sm);
}

// ---- 3. features --------------------------------------------------------------------------------------
// blockIdx.x: the column; a thread per feature, its gridDim.y * 64 * kQyWaves threads striding over them
__global__ __launch_bounds__(64 * kQyWaves) void query_features_kernel(const uint8_t* __restrict__ dec,
                                                                       const covt_geom_desc* __restrict__ gdescs,
                                                                       const uint8_t* __restrict__ asmb,
                                                                       const covt_geom_result* __restrict__ gres,
                                                                       const covt_select_desc* __restrict__ sdescs,
                                                                       uint8_t* select, QueryArgs q) {
    const int64_t col = blockIdx.x;
    const covt_geom_desc gd = gdescs[col];
    const covt_geom_result gr = gres[col];
    const covt_select_desc sd = sdescs[col];
    const int32_t threads = (int32_t)(gridDim.y * 64 * kQyWaves);
    if (query_col_status(gd, gr, sd) != COVT_OK) {
        // the column rule: an all-zero mask in both modes (nothing at a negative offset)
        if (sd.off < 0) return;
        uint8_t* const mask = select + sd.off + select_mask_off(sd.n_features);
        for (int32_t f = (int32_t)(blockIdx.y * 64 * kQyWaves + threadIdx.x); f < sd.n_features; f += threads)
            ((gw_u8*)mask)[f] = 0;
        return;
    }
    const QueryCol c = query_column(gd, gr, sd, dec, asmb, select);
    const g_u8* const ring_bits = (const g_u8*)c.ring_bits;
    const bool none = query_inverted(q.w);
    const int l = lane_id();
    // (every lane of a wave runs the same number of steps: the wave finishes its wide features together)
    for (int32_t f0 = (int32_t)(blockIdx.y * 64 * kQyWaves + (threadIdx.x & ~63u)); f0 < c.n; f0 += threads) {
        const int32_t f = f0 + l;
        const bool have = f < c.n;
        int32_t r0 = 0, r1 = 0;
        uint32_t t = 0, v = 0;
        bool coords = false;
        if (have) {
            r0 = c.part_at(c.geo_at(f)), r1 = c.part_at(c.geo_at(f + 1));
            t = (uint32_t)((const g_u8*)c.types)[f];
            coords = c.ring_at(r1) > c.ring_at(r0);
        }
        const bool wide = have && r1 - r0 >= kQyNarrow;
        if (have && !wide)
            for (int32_t r = r0; r < r1; ++r) v = query_join(v, (uint32_t)ring_bits[r]);
        // the wide features of this step, one after the other by the whole wave
        wave_each(wide, [&](int src) {
            const int32_t wr0 = (int32_t)lane_bcast((uint32_t)r0, src), wr1 = (int32_t)lane_bcast((uint32_t)r1, src);
            uint32_t part = 0;
            for (int32_t r = wr0 + l; r < wr1; r += 64) part = query_join(part, (uint32_t)ring_bits[r]);
            part = seg_wave_join<QueryV>(part);
            if (l == src) v = part;
        });
        if (have) {
            bool keep = !none && query_feature(v, t, coords, q.relation);
            if (q.mode == COVT_WHERE_AND) keep = keep && ((const g_u8*)c.mask)[f] != 0;
            ((gw_u8*)c.mask)[f] = keep ? 1 : 0;
        }
    }
}

}  // namespace covt

extern "C" void covt_select_query_init(covt_select_query* query) {
    if (!query) return;
    *query = covt_select_query{};
    query->size = (uint32_t)sizeof(covt_select_query);
    query->relation = COVT_QUERY_INTERSECTS;
}

extern "C" int covt_select_query_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                        const covt_geom_result* d_gres, const covt_select_desc* d_sdesc,
                                        int64_t n_columns, const covt_select_query* query, int32_t mode,
                                        uint8_t* d_select, int32_t* d_status, void* hip_stream) {
    using namespace covt;
    if (n_columns < 0 || !query_valid(query) || (mode != COVT_WHERE_WRITE && mode != COVT_WHERE_AND))
        return COVT_ERR_INVALID_ARG;
    if (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_sdesc || !d_select)) return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || ((uintptr_t)d_select & 15)) return COVT_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)hip_stream;
    const QueryArgs q{query_window(*query), query->relation, mode};
    if (d_status)
        hipLaunchKernelGGL(query_init_kernel, dim3((unsigned)((n_columns + 255) / 256)), dim3(256), 0, s, d_gdesc, d_gres,
                           d_sdesc, n_columns, d_status);
    const dim3 grid((unsigned)n_columns, product_blocks_y(n_columns));
    hipLaunchKernelGGL(query_rings_kernel, grid, dim3(64 * kQyWaves), 0, s, d_gdesc, d_asm, d_gres, d_sdesc, d_select, q);
    hipLaunchKernelGGL(query_features_kernel, grid, dim3(64 * kQyWaves), 0, s, d_decoded, d_gdesc, d_asm, d_gres, d_sdesc,
                       d_select, q);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

// covt_simplify.hip -- gfx950 geometry simplification of assembled geometry columns (include/covt.h "Geometry
// simplification"): snap to the grid of 2^s, drop the coordinates that repeat their predecessor, empty the rings
// and lines that collapsed; the output is another assembled column in the simplify buffer.
//
// Six launches; no allocation, no atomics, every output element written exactly once by one thread (so a
// captured graph replays the pass as it is and the bytes do not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's and the shift's), its part and ring counts.
//   2. rings: the segmented reduction of covt_segscan.h over the rings' edges (seg_run under RingEdgePolicy),
//      the value a count: an edge's term (SpEdge) is 1 if its two coordinates snap differently.  A non-empty
//      ring's k_r = 1 + the sum goes to ring_k[r] in the column's scratch.
//   3. features: a thread per feature, the whole wave (a lane per part) for those of kSpNarrow parts or rings.
//      It applies the type minima and the shell rule part by part and stores k'_r over k_r, bit 31 set for
//      the rings of POINT / MULTIPOINT features (k'_r their length: every coordinate is kept).
//   4. count: the coordinates in chunks of COVT_SIMPLIFY_CHUNK, each with its ring and its predecessor
//      (ring_stream of covt_segscan.h); kept iff its ring stands and it is a point, its ring's first or differs
//      from its predecessor.  The chunk's kept count goes to chunk_k[chunk].
//   5. scan: per column (a workgroup in small batches, a wave in large ones) the exclusive scan of k'_r ->
//      ring_offsets' and num_coords, the exclusive scan of chunk_k in place (StepScan of covt_coop.h), the copy
//      of the two upper levels.
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
constexpr uint32_t kSpPoints = 0x80000000u;  // ring_k: a ring of a POINT / MULTIPOINT feature

struct SpCol : GeomCol {
    const uint8_t* types;
    int32_t *o_geo, *o_part, *o_ring, *o_xy;  // the simplified column
    uint32_t *ring_k, *chunk_k;               // the scratch
    int32_t coord_cap;
    int32_t s;  // the shift

    __device__ __forceinline__ int32_t snap(int32_t v) const { return simplify_snap(v, s); }
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

// what the rings pass supplies to RingEdgePolicy: the snapped coordinates, 1 for an edge whose ends differ, the
// count of a non-empty ring's edges + 1
struct SpEdge {
    typedef AddV<uint32_t> V;
    const SpCol& c;
    __device__ __forceinline__ int32_t map(int32_t v) const { return c.snap(v); }
    __device__ __forceinline__ uint32_t edge(int32_t x0, int32_t y0, int32_t x1, int32_t y1) const {
        return x0 != x1 || y0 != y1 ? 1u : 0u;
    }
    __device__ __forceinline__ void put(int32_t r, uint32_t v, bool any) const {
        ((gw_u32*)c.ring_k)[r] = any ? v + 1u : 0u;
    }
};
typedef RingEdgePolicy<SpEdge, kSpWaves> SpRings;

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
    __shared__ SegSmem<SpRings> sm;
    const int64_t col = blockIdx.x;
    if (ores[col].status != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, sp_shift(shift, d_shift, col));
    const SpEdge e{c};
    SpRings p{c, e};
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
        wave_each(wide, [&](int src) {
            const int32_t wg0 = (int32_t)lane_bcast((uint32_t)g0, src), wg1 = (int32_t)lane_bcast((uint32_t)g1, src);
            const uint32_t wt = lane_bcast(t, src);
            for (int32_t g = wg0 + l; g < wg1; g += 64) sp_part(c, g, wt);
        });
    }
}

// ---- 4. count, 6. write -------------------------------------------------------------------------------
// whether a coordinate that snaps to (x, y) after (bx, by) is kept; r its ring, head: it is the ring's first
__device__ __forceinline__ bool sp_keep(const SpCol& c, int32_t r, bool head, int32_t x, int32_t y, int32_t bx, int32_t by) {
    const uint32_t k = ((g_u32*)c.ring_k)[r];
    return (k & ~kSpPoints) != 0u && ((k & kSpPoints) != 0u || head || x != bx || y != by);
}

// blockIdx.x: the column; the walk is ring_stream's, the row here: the kept coordinates' ballots are the row's
// count and, WRITE, a kept coordinate's rank in the row.
template <bool WRITE>
__global__ __launch_bounds__(64 * kSpWaves) void simplify_stream_kernel(
    const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb, const covt_geom_result* __restrict__ gres,
    const covt_simplify_desc* __restrict__ sdescs, int32_t shift, const int32_t* __restrict__ d_shift,
    uint8_t* __restrict__ out, const covt_geom_result* __restrict__ ores) {
    __shared__ __attribute__((aligned(16))) uint32_t marks[kSpWaves][128];
    const int64_t col = blockIdx.x;
    if (ores[col].status != COVT_OK) return;
    const SpCol c = sp_column(gdescs[col], gres[col], sdescs[col], nullptr, asmb, out, sp_shift(shift, d_shift, col));
    ring_stream<COVT_SIMPLIFY_CHUNK, kSpWaves, WRITE>(
        c, c.chunk_k, marks[threadIdx.x >> 6], [&](int32_t v) { return c.snap(v); }, [&](const RingRow& w) {
            const bool k0 = w.i0 < w.B && sp_keep(c, w.r0, w.m0 != 0u, w.x0, w.y0, w.bx, w.by);
            const bool k1 = w.i0 + 1 < w.B && sp_keep(c, w.r1, w.m1 != 0u, w.x1, w.y1, w.x0, w.y0);
            const uint64_t b0 = __ballot(k0), b1 = __ballot(k1);
            if (WRITE) {
                // (a destination is below the column's kept count, itself at most V; checked all the same)
                const uint32_t d0 = w.run + (uint32_t)(bits_below(b0) + bits_below(b1)), d1 = d0 + (k0 ? 1u : 0u);
                if (k0 && d0 < (uint32_t)c.coord_cap)
                    *(gw_u64*)(c.o_xy + 2 * (int64_t)d0) = (uint64_t)(uint32_t)w.x0 | ((uint64_t)(uint32_t)w.y0 << 32);
                if (k1 && d1 < (uint32_t)c.coord_cap)
                    *(gw_u64*)(c.o_xy + 2 * (int64_t)d1) = (uint64_t)(uint32_t)w.x1 | ((uint64_t)(uint32_t)w.y1 << 32);
            }
            return (uint32_t)(__popcll(b0) + __popcll(b1));
        });
}

// ---- 5. scan ------------------------------------------------------------------------------------------
// ring_offsets' and num_coords from k'_r, chunk_k -> its exclusive scan in place, the upper two levels copied
template <int NW>
__device__ void simplify_scan_column(const SpCol& c, covt_geom_result* res, AsmSmemT<NW, kSpIpl>& sm) {
    const int l = Coop<NW, kSpIpl>::tid();
    const uint32_t cap = (uint32_t)c.coord_cap;
    StepScan<NW, kSpIpl> scan{sm};
    const uint32_t kept = scan.run(
        c.R, [&](int32_t r) { return ((g_u32*)c.ring_k)[r] & ~kSpPoints; },
        [&](int32_t r, uint32_t before) { ((gw_i32*)c.o_ring)[r] = (int32_t)min(before, cap); });
    if (l == 0) {  // (the kept counts of a well-formed column sum to at most V)
        ((gw_i32*)c.o_ring)[c.R] = (int32_t)min(kept, cap);
        res->num_coords = (int32_t)min(kept, cap);
    }
    scan.in_place(c.chunk_k, ring_chunks<COVT_SIMPLIFY_CHUNK>(c));
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

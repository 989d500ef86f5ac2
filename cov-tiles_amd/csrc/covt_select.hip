// covt_select.hip -- gfx950 feature selection over WKB columns (include/covt.h "Feature selection"): a keep
// mask per feature -> the selection vector and the compacted WKB column; and the predicate pass that writes the
// mask from the bounding boxes and the measures.
//
// The predicate is one kernel: a thread per feature, the column's bounding-box (and measures) arrays loaded as
// they lie, comparisons only, one byte stored.
//
// The selection is two kernels per launch, no scratch, no look-back, no atomics (so a captured graph replays
// as it is and the bytes do not depend on scheduling):
//
//   1. scan: the exclusive scan of the pair (kept count, kept bytes) over the column's features; kept
//      feature f of rank j stores sel[j] = f and offsets[j], the column's last step offsets[n_selected] and the
//      result.  One wave per column in a large batch, a workgroup of kSelCoopWaves waves per column in a small
//      one (Coop / excl_scan4 of covt_coop.h, the shape of the WKB size scan).
//   2. copy: a segmented gather copy over the OUTPUT bytes, so a column of 21-byte POINT values costs what
//      its bytes cost, not a wave per value.  The column's [0, n_bytes) is cut into chunks of kSelChunk bytes
//      (64 lanes x 16); every wave of the column's gridDim.y workgroups (sized from the batch as the WKB write
//      pass is) takes a run of consecutive chunks.  A byte's owner is the last j with offsets[j] <= b: the wave
//      finds its first owner with a 64-ary search (seg_first_at), stages the kSelWin offsets that follow and
//      the source offsets wkb_offsets[sel[.]] of those values in LDS, keeps that window while it covers the
//      chunk, and a lane whose owner lies past the window searches global memory.  The slice's bytes member is
//      16-byte aligned and the output is contiguous, so every destination vector is one aligned 16-byte store;
//      a vector inside one value is one unaligned 16-byte load (gfx950 runs with unaligned access mode on, as
//      covt_wkb.hip relies on), a vector that crosses values takes one such load per value it touches, placed
//      so that the value's piece lands where it belongs and masked in (byte by byte where that load would
//      leave the source column: its first and last 15 bytes).  No byte past the source column's n_bytes is
//      read and none past the output's n_bytes written: the tail vector goes out as dwords and bytes.
//
// wkb_offsets are read clamped to [0, the source's n_bytes] (SelCol::src_at), in the scan and in the copy
// alike, and the scan fails a column whose kept lengths then pass that total: whatever the offsets hold, every
// source address lies inside the source slice and every destination address inside the select slice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_bbox_plan.h"
#include "covt_coop.h"
#include "covt_measures_plan.h"
#include "covt_segscan.h"
#include "covt_select_plan.h"
#include "covt_wave.h"

namespace covt {

constexpr int kSelCoopWaves = 16;         // scan, small batches: waves per column
constexpr int kSelCoopMaxColumns = 4096;  // batches of at most this many columns are "small"
constexpr int kSelIpl = 4;                // scan: features per thread and step
constexpr int kSelWaves = 4;              // waves per workgroup (predicate, wave-per-column scan, copy)
constexpr int kSelChunk = 64 * 16;        // copy: output bytes per wave chunk, 16 per lane
constexpr int kSelWin = 256;              // copy: owners staged in LDS per window (a multiple of 64)

// ---- the predicate -------------------------------------------------------------------------------------
// small batches: blockIdx.x the column, its features over gridDim.y workgroups; large ones: a wave per column
__global__ __launch_bounds__(64 * kSelWaves) void sel_predicate_kernel(
    const covt_bbox_desc* __restrict__ bdescs, const uint8_t* __restrict__ bbox,
    const covt_bbox_result* __restrict__ bres, const covt_measures_desc* __restrict__ mdescs,
    const uint8_t* __restrict__ measures, const covt_measures_result* __restrict__ mres,
    const covt_select_desc* __restrict__ sdescs, int64_t n_cols, covt_select_pred pred, uint8_t* __restrict__ select,
    int wave_per_column) {
    int64_t col;
    int32_t first, stride;
    if (wave_per_column) {
        col = uni64((int64_t)blockIdx.x * kSelWaves + (threadIdx.x >> 6));
        first = lane_id();
        stride = 64;
    } else {
        col = blockIdx.x;
        first = (int32_t)(blockIdx.y * blockDim.x + threadIdx.x);
        stride = (int32_t)(gridDim.y * blockDim.x);
    }
    if (col >= n_cols) return;
    const covt_select_desc sd = sdescs[col];
    const int32_t n = sd.n_features;
    if ((sd.flags & COVT_SELECT_TOO_LARGE) || n <= 0) return;
    const covt_bbox_desc bd = bdescs[col];
    const bool window = (pred.flags & COVT_SELECT_WINDOW) != 0, size = (pred.flags & COVT_SELECT_MIN_SIZE) != 0;
    // a column without boxes (or, asked for, without measures) keeps nothing
    bool ok = bres[col].status == COVT_OK && bd.n_features == n && bd.flags == 0;
    const double* area = nullptr;
    const double* length = nullptr;
    if (size) {
        const covt_measures_desc md = mdescs[col];
        ok = ok && mres[col].status == COVT_OK && md.n_features == n && md.flags == 0;
        area = (const double*)(measures + md.off + measures_area_off(n));
        length = (const double*)(measures + md.off + measures_length_off(n));
    }
    const uint8_t* box = bbox + bd.off;
    uint8_t* mask = select + sd.off + select_mask_off(n);
    for (int32_t f = first; f < n; f += stride) {
        uint8_t m = 0;
        if (ok) {
            const double xmin = ((g_f64*)(box + bbox_array_off(n, 0)))[f];
            double ymin = 0.0, xmax = 0.0, ymax = 0.0, a = 0.0, len = 0.0;
            if (window) {
                ymin = ((g_f64*)(box + bbox_array_off(n, 1)))[f];
                xmax = ((g_f64*)(box + bbox_array_off(n, 2)))[f];
                ymax = ((g_f64*)(box + bbox_array_off(n, 3)))[f];
            }
            if (size) {
                a = ((g_f64*)area)[f];
                len = ((g_f64*)length)[f];
            }
            m = select_keep(pred, xmin, ymin, xmax, ymax, a, len);
        }
        ((gw_u8*)mask)[f] = m;
    }
}

// ---- the column ----------------------------------------------------------------------------------------
struct SelCol {
    const int32_t* woff;  // the source: wkb_offsets, wkb_bytes
    const uint8_t* wbytes;
    const uint8_t* mask;
    int32_t *sel, *offs;
    uint8_t* bytes;
    int32_t n;
    int32_t src_nb;  // the source column's byte count

    // wkb_offsets[f] inside [0, src_nb]
    __device__ __forceinline__ int32_t src_at(int32_t f) const { return clamp0(((const g_i32*)woff)[f], src_nb); }
    __device__ __forceinline__ int32_t sel_at(int32_t j) const { return ((const g_i32*)sel)[j]; }
    __device__ __forceinline__ int32_t offs_at(int32_t j) const { return ((const g_i32*)offs)[j]; }
};
__device__ __forceinline__ SelCol sel_col(const covt_wkb_desc& wd, const covt_wkb_result& wr, const uint8_t* wkb,
                                          const covt_select_desc& sd, uint8_t* select) {
    SelCol c;
    c.woff = (const int32_t*)(wkb + wd.offsets_off);
    c.wbytes = wkb + wd.bytes_off;
    c.n = sd.n_features;
    uint8_t* base = select + sd.off;
    c.mask = base + select_mask_off(c.n);
    c.sel = (int32_t*)(base + select_sel_off(c.n));
    c.offs = (int32_t*)(base + select_offsets_off(c.n));
    c.bytes = base + select_bytes_off(c.n);
    c.src_nb = (int32_t)wr.n_bytes;
    return c;
}

// the column's status before any work: the WKB pass's, then the two layouts' (one capacity, an int32 offset,
// that holds the source's bytes; one feature count)
__device__ __forceinline__ int32_t sel_precheck(const covt_wkb_desc& wd, const covt_wkb_result& wr,
                                                const covt_select_desc& sd) {
    return product_precheck(wr.status, (wd.flags & COVT_WKB_TOO_LARGE) || (sd.flags & COVT_SELECT_TOO_LARGE),
                            sd.byte_cap == wd.byte_cap && sd.byte_cap >= 0 && sd.byte_cap <= INT32_MAX &&
                                wr.n_bytes >= 0 && wr.n_bytes <= sd.byte_cap,
                            sd.n_features == wd.n_features && sd.n_features >= 0);
}

// ---- 1. scan -------------------------------------------------------------------------------------------
// (the stepped loop written out, not StepScan of covt_coop.h: a step scans two values, count and bytes, from one
// set of loads, and a kept feature's store needs both prefixes)
template <int NW, int IPL>
__device__ void sel_scan_column(const covt_wkb_desc& wd, const covt_wkb_result& wr, const uint8_t* __restrict__ wkb,
                                const covt_select_desc& sd, uint8_t* __restrict__ select, covt_select_result& res,
                                AsmSmemT<NW, IPL>& sm) {
    constexpr int K = Coop<NW, IPL>::K;
    const int l = Coop<NW, IPL>::tid();
    auto ioff = [&](int k) { return NW == 1 ? 64 * k + l : IPL * l + k; };
    res.n_selected = 0;
    res.n_bytes = 0;
    res.status = sel_precheck(wd, wr, sd);
    if (res.status != COVT_OK) return;
    const SelCol c = sel_col(wd, wr, wkb, sd, select);
    int buf = 0;
    uint32_t J = 0, B = 0;  // kept features and their bytes before this step
    for (int32_t f0 = 0; f0 < c.n; f0 += K) {
        uint32_t keep[IPL], len[IPL], ej[IPL], eb[IPL], tj, tb;
#pragma unroll
        for (int k = 0; k < IPL; ++k) {
            const int32_t f = f0 + ioff(k);
            keep[k] = f < c.n && ((const g_u8*)c.mask)[f] != 0 ? 1u : 0u;
            len[k] = keep[k] ? (uint32_t)max(c.src_at(f + 1) - c.src_at(f), 0) : 0u;
        }
        excl_scan4(sm, buf, keep, ej, tj);
        excl_scan4(sm, buf, len, eb, tb);
#pragma unroll
        for (int k = 0; k < IPL; ++k) {
            if (!keep[k]) continue;
            const uint32_t j = J + ej[k];  // (below n_features: a rank)
            ((gw_i32*)c.sel)[j] = f0 + ioff(k);
            ((gw_i32*)c.offs)[j] = (int32_t)add_sat(B, eb[k]);  // (saturated only in a column that fails below)
        }
        J += tj;
        B = add_sat(B, tb);
    }
    if (B > (uint32_t)c.src_nb) {  // (never with the offsets a WKB pass wrote)
        res.status = COVT_ERR_COUNT_MISMATCH;
        return;
    }
    if (l == 0) ((gw_i32*)c.offs)[J] = (int32_t)B;
    res.n_selected = (int32_t)J;
    res.n_bytes = (int64_t)B;
}

// one wave per column
__global__ __launch_bounds__(64 * kSelWaves) void sel_scan_kernel(
    const covt_wkb_desc* __restrict__ wdescs, const uint8_t* __restrict__ wkb, const covt_wkb_result* __restrict__ wres,
    const covt_select_desc* __restrict__ sdescs, int64_t n_cols, uint8_t* __restrict__ select,
    covt_select_result* __restrict__ sres) {
    __shared__ AsmSmemT<1, kSelIpl> smem[kSelWaves];
    const int w = threadIdx.x >> 6;
    const int64_t c = uni64((int64_t)blockIdx.x * kSelWaves + w);
    if (c >= n_cols) return;
    const covt_wkb_desc wd = wdescs[c];
    const covt_wkb_result wr = wres[c];
    const covt_select_desc sd = sdescs[c];
    covt_select_result r;
    sel_scan_column<1, kSelIpl>(wd, wr, wkb, sd, select, r, smem[w]);
    if (lane_id() == 0) sres[c] = r;
}

// a workgroup per column (small batches: a long column's scan in steps of 4096 features)
__global__ __launch_bounds__(64 * kSelCoopWaves) void sel_scan_coop_kernel(
    const covt_wkb_desc* __restrict__ wdescs, const uint8_t* __restrict__ wkb, const covt_wkb_result* __restrict__ wres,
    const covt_select_desc* __restrict__ sdescs, int64_t n_cols, uint8_t* __restrict__ select,
    covt_select_result* __restrict__ sres) {
    __shared__ AsmSmemT<kSelCoopWaves, kSelIpl> smem;
    const int64_t c = blockIdx.x;
    if (c >= n_cols) return;
    const covt_wkb_desc wd = wdescs[c];
    const covt_wkb_result wr = wres[c];
    const covt_select_desc sd = sdescs[c];
    covt_select_result r;
    sel_scan_column<kSelCoopWaves, kSelIpl>(wd, wr, wkb, sd, select, r, smem);
    if (threadIdx.x == 0) sres[c] = r;
}

// ---- 2. copy -------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) SelSmem {
    int32_t off[kSelWin];  // offsets[ws ..] of one wave's window (past offsets[n_selected]: INT32_MAX)
    int32_t src[kSelWin];  // the source offsets of those values
};

// The owners of a wave's bytes: offsets[ws .. ws + kSelWin) and the values' source offsets staged in LDS, ws
// an owner at or before the wave's next byte.  Entries outside the window are read from global memory.
struct SelWindow {
    const SelCol& c;
    int32_t* off;
    int32_t* src;
    int32_t n_sel;
    int32_t ws;

    // stage the window from ws on; wave_sync before use
    __device__ __forceinline__ void load() const {
#pragma unroll
        for (int k = 0; k < kSelWin / 64; ++k) {
            const int32_t i = ws + 64 * k + lane_id();
            off[64 * k + lane_id()] = i <= n_sel ? c.offs_at(i) : 0x7fffffff;
            src[64 * k + lane_id()] = i < n_sel ? c.src_at(c.sel_at(i)) : 0;
        }
    }
    // the window holds the end of byte x's value
    __device__ __forceinline__ bool covers(int32_t x) const { return off[kSelWin - 1] > x; }
    // offsets[i], i in [ws, n_sel]
    __device__ __forceinline__ int32_t offs_at(int32_t i) const {
        return (uint32_t)(i - ws) < (uint32_t)kSelWin ? off[i - ws] : c.offs_at(i);
    }
    // the source offset of value j, j in [ws, n_sel)
    __device__ __forceinline__ int32_t src_of(int32_t j) const {
        return (uint32_t)(j - ws) < (uint32_t)kSelWin ? src[j - ws] : c.src_at(c.sel_at(j));
    }
    // the last j with offsets[j] <= x, for x in [offsets[ws], n_bytes)
    __device__ __forceinline__ int32_t owner(int32_t x) const {
        int32_t a, b;
        if (covers(x)) {
            a = ws, b = ws + kSelWin - 2;
            while (a < b) {
                const int32_t mid = (a + b + 1) >> 1;
                if (off[mid - ws] <= x) a = mid;
                else b = mid - 1;
            }
            return a;
        }
        // (the window's last entry is a real offset at or below x, so its value exists: ws + kSelWin - 1 < n_sel)
        a = ws + kSelWin - 1, b = n_sel - 1;
        while (a < b) {
            const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b + 1u) >> 1);
            if (c.offs_at(mid) <= x) a = mid;
            else b = mid - 1;
        }
        return a;
    }
};

// a lane's walk through the values of its vector: value j = output bytes [o0, o1)
struct SelCursor {
    int32_t j, o0, o1;
    // on to the value that holds byte p (p below n_bytes = offsets[n_sel]; values of no bytes are passed over)
    __device__ __forceinline__ void seek(const SelWindow& w, uint32_t p) {
        while ((uint32_t)o1 <= p && j + 1 < w.n_sel) {
            ++j;
            o0 = o1;
            o1 = w.offs_at(j + 1);
        }
    }
    // where byte p of the output lies in the source
    __device__ __forceinline__ const uint8_t* at(const SelWindow& w, uint32_t p) const {
        return w.c.wbytes + (uint32_t)w.src_of(j) + (p - (uint32_t)o0);
    }
};

// one wave, one chunk of output bytes [base, base + L), 1 <= L <= kSelChunk; returns the owner of the last
// lane's first byte, at or before the next chunk's first owner (uniform)
__device__ __forceinline__ int32_t sel_copy_chunk(const SelWindow& w, uint32_t base, uint32_t L, uint32_t nb) {
    const uint32_t b = base + 16u * (uint32_t)lane_id();
    const bool active = 16u * (uint32_t)lane_id() < L;
    SelCursor cur;
    cur.j = active ? w.owner((int32_t)b) : w.ws;
    const int32_t hint = (int32_t)lane_bcast((uint32_t)cur.j, (int)((L - 1u) >> 4));
    if (!active) return hint;
    cur.o0 = w.offs_at(cur.j);
    cur.o1 = w.offs_at(cur.j + 1);
    uint8_t* dst = w.c.bytes + b;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if ((uint32_t)cur.o1 >= b + 16u) {  // the vector lies inside one value
        const u32x4 q = *(g_u32x4u*)cur.at(w, b);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        // The vector's pieces, one per value it touches: a piece at bytes [a, e) of the vector comes out of one
        // unaligned 16-byte load placed so that the piece lands at [a, e), masked in dword by dword.  Where that
        // load would leave the source column's bytes (its first and last 15 bytes) the piece goes byte by byte.
        const uint32_t end = min(b + 16u, nb);
        uint32_t pos = b;
        while (pos < end) {
            cur.seek(w, pos);
            const uint32_t pe = max(min((uint32_t)cur.o1, end), pos + 1u);
            const uint32_t a = pos - b, e = pe - b;
            const int32_t so = w.src_of(cur.j) + (int32_t)(pos - (uint32_t)cur.o0) - (int32_t)a;  // of vector byte 0
            if (so >= 0 && so <= w.c.src_nb - 16) {
                const u32x4 q = *(g_u32x4u*)(w.c.wbytes + so);
                const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // bytes [lo, hi) of dword k belong to the piece
                    const uint32_t lo = min(max((int32_t)a - 4 * k, 0), 4), hi = min(max((int32_t)e - 4 * k, 0), 4);
                    const uint32_t m = (uint32_t)((1ull << (8u * hi)) - 1ull) & ~(uint32_t)((1ull << (8u * lo)) - 1ull);
                    v[k] |= qq[k] & m;
                }
            } else {
                for (uint32_t i = a; i < e; ++i) {
                    const uint32_t byte = (uint32_t)*(const g_u8*)(w.c.wbytes + clamp0(so + (int32_t)i, w.c.src_nb - 1)) << (8u * (i & 3u));
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] |= (i >> 2) == (uint32_t)k ? byte : 0u;
                }
            }
            pos = pe;
        }
    }
    if (b + 16u <= nb) {
        *(gw_u32x4*)dst = u32x4{v[0], v[1], v[2], v[3]};
        return hint;
    }
    // the column's tail vector: whole dwords, then bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t p = b + 4u * k;
        if (p + 4u <= nb) {
            *(gw_u32*)(dst + 4 * k) = v[k];
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (p + t < nb) *(gw_u8*)(dst + 4 * k + t) = (uint8_t)(v[k] >> (8 * t));
        }
    }
    return hint;
}

// blockIdx.x: the column; each of its gridDim.y * kSelWaves waves takes a run of consecutive chunks of the
// output bytes
__global__ __launch_bounds__(64 * kSelWaves) void sel_copy_kernel(
    const covt_wkb_desc* __restrict__ wdescs, const uint8_t* __restrict__ wkb, const covt_wkb_result* __restrict__ wres,
    const covt_select_desc* __restrict__ sdescs, uint8_t* __restrict__ select,
    const covt_select_result* __restrict__ sres) {
    __shared__ SelSmem smem[kSelWaves];
    const int64_t col = blockIdx.x;
    const covt_select_result sr = sres[col];  // (the scan's, earlier on this stream)
    if (sr.status != COVT_OK || sr.n_bytes <= 0 || sr.n_selected <= 0) return;
    const covt_wkb_desc wd = wdescs[col];
    const covt_wkb_result wr = wres[col];
    const covt_select_desc sd = sdescs[col];
    const SelCol c = sel_col(wd, wr, wkb, sd, select);
    const uint32_t nb = (uint32_t)sr.n_bytes;
    const int w = threadIdx.x >> 6;
    const int32_t wave = uni((int32_t)(blockIdx.y * kSelWaves + w));
    const int32_t waves = (int32_t)(gridDim.y * kSelWaves);
    const int64_t chunks = ((int64_t)nb + kSelChunk - 1) / kSelChunk;
    const int32_t cb = (int32_t)(chunks * wave / waves), ce = (int32_t)(chunks * (wave + 1) / waves);
    if (cb >= ce) return;
    SelWindow win{c, smem[w].off, smem[w].src, sr.n_selected, 0};
    // the owner of the run's first byte: the last j with offsets[j] <= b
    const int32_t first = cb * kSelChunk;
    int32_t hint = seg_first_at(sr.n_selected, first + 1, [&](int32_t j) { return c.offs_at(j); }) - 1;
    bool have = false;
    for (int32_t j = cb; j < ce; ++j) {
        const uint32_t base = (uint32_t)j * kSelChunk, L = min((uint32_t)kSelChunk, nb - base);
        // the window is kept while it holds the end of the chunk's last value
        if (!have || uni(win.off[kSelWin - 1]) <= (int32_t)(base + L - 1u)) {
            wave_sync();  // (the window is read by the previous chunk)
            win.ws = hint;
            win.load();
            wave_sync();
            have = true;
        }
        hint = uni(sel_copy_chunk(win, base, L, nb));
    }
}

int predicate_launch(const covt_bbox_desc* d_bdesc, const uint8_t* d_bbox, const covt_bbox_result* d_bres,
                     const covt_measures_desc* d_mdesc, const uint8_t* d_measures, const covt_measures_result* d_mres,
                     const covt_select_desc* d_sdesc, int64_t n_columns, const covt_select_pred& pred, uint8_t* d_select,
                     hipStream_t s) {
    const bool small = n_columns <= kSelCoopMaxColumns;
    const dim3 grid = small ? dim3((unsigned)n_columns, product_blocks_y(n_columns))
                            : dim3((unsigned)((n_columns + kSelWaves - 1) / kSelWaves));
    hipLaunchKernelGGL(sel_predicate_kernel, grid, dim3(64 * kSelWaves), 0, s, d_bdesc, d_bbox, d_bres, d_mdesc,
                       d_measures, d_mres, d_sdesc, n_columns, pred, d_select, small ? 0 : 1);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

int select_launch(const covt_wkb_desc* d_wdesc, const uint8_t* d_wkb, const covt_wkb_result* d_wres,
                  const covt_select_desc* d_sdesc, int64_t n_columns, uint8_t* d_select, covt_select_result* d_sres,
                  hipStream_t s) {
    const bool small = n_columns <= kSelCoopMaxColumns;
    if (small) {
        hipLaunchKernelGGL(sel_scan_coop_kernel, dim3((unsigned)n_columns), dim3(64 * kSelCoopWaves), 0, s, d_wdesc,
                           d_wkb, d_wres, d_sdesc, n_columns, d_select, d_sres);
    } else {
        const int64_t blocks = (n_columns + kSelWaves - 1) / kSelWaves;
        hipLaunchKernelGGL(sel_scan_kernel, dim3((unsigned)blocks), dim3(64 * kSelWaves), 0, s, d_wdesc, d_wkb, d_wres,
                           d_sdesc, n_columns, d_select, d_sres);
    }
    const unsigned gy = small ? product_blocks_y(n_columns) : 1u;
    hipLaunchKernelGGL(sel_copy_kernel, dim3((unsigned)n_columns, gy), dim3(64 * kSelWaves), 0, s, d_wdesc, d_wkb,
                       d_wres, d_sdesc, d_select, d_sres);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

}  // namespace covt

extern "C" void covt_select_pred_init(covt_select_pred* pred) {
    if (!pred) return;
    *pred = covt_select_pred{};
    pred->size = (uint32_t)sizeof(covt_select_pred);
}

extern "C" int covt_select_predicate_device(const covt_bbox_desc* d_bdesc, const uint8_t* d_bbox,
                                            const covt_bbox_result* d_bres, const covt_measures_desc* d_mdesc,
                                            const uint8_t* d_measures, const covt_measures_result* d_mres,
                                            const covt_select_desc* d_sdesc, int64_t n_columns,
                                            const covt_select_pred* pred, uint8_t* d_select, void* hip_stream) {
    if (n_columns < 0 || !select_pred_valid(pred)) return COVT_ERR_INVALID_ARG;
    const bool size = (pred->flags & COVT_SELECT_MIN_SIZE) != 0;
    if (n_columns && (!d_bdesc || !d_bbox || !d_bres || !d_sdesc || !d_select ||
                      (size && (!d_mdesc || !d_measures || !d_mres))))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || ((uintptr_t)d_select & 15)) return COVT_ERR_INVALID_ARG;
    return covt::predicate_launch(d_bdesc, d_bbox, d_bres, d_mdesc, d_measures, d_mres, d_sdesc, n_columns, *pred,
                                  d_select, (hipStream_t)hip_stream);
}

extern "C" int covt_geometry_select_device(const covt_wkb_desc* d_wdesc, const uint8_t* d_wkb,
                                           const covt_wkb_result* d_wres, const covt_select_desc* d_sdesc,
                                           int64_t n_columns, uint8_t* d_select, covt_select_result* d_sres,
                                           void* hip_stream) {
    if (n_columns < 0 || (n_columns && (!d_wdesc || !d_wkb || !d_wres || !d_sdesc || !d_select || !d_sres)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || ((uintptr_t)d_select & 15)) return COVT_ERR_INVALID_ARG;
    return covt::select_launch(d_wdesc, d_wkb, d_wres, d_sdesc, n_columns, d_select, d_sres, (hipStream_t)hip_stream);
}

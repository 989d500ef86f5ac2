// covt_where.hip -- gfx950 property predicates (include/covt.h "Property predicates"): a conjunction of clauses
// over the materialized property columns, evaluated per feature, written into the keep masks of the select
// buffer (or ANDed into them).  The rules are covt_where_plan.h's; this file is the launch and the memory shape.
//
// One kernel, the launch shape of sel_predicate_kernel: in a batch of at most kWhereCoopMaxColumns columns
// blockIdx.x is the column and its features go over gridDim.y workgroups; in a larger one a wave takes a column.
// The group (workgroup or wave) of a column first resolves the clauses for that column into LDS (WhereCol: the
// clause header, the bound property column's members, its type), so the feature loop reads uniform LDS words
// and no descriptor.  The blob itself is staged into LDS once per workgroup, 2,320 bytes, and read there
// clamped to its own arrays.
//
// A lane takes four consecutive features: one validity nibble, one 16-byte vector of int32 / float values (two
// for int64), in AND mode one mask dword, and one mask dword stored (the mask member starts 16-byte aligned; the
// column's tail goes out as bytes).  Every member of a property column is padded to 16 bytes
// (prop_layout_sizes), so the value vector of the column's last features stays inside the member.
//
// Strings.  For a clause bound to a STRING column of at most kWhereDictBitsGroup entries (kWhereDictBitsWave in
// a wave-per-column launch, and there only while the dictionary is no longer than kWhereDictPerFeature entries
// per feature) the group first builds a match bitmap over the dictionary in LDS: lanes over entries, lengths
// compared first and bytes only on a length hit, a wave's 64 verdicts stored as one ballot (no LDS atomics).
// A feature is then one LDS bit probe.  Otherwise each present feature compares its own entry.  Both use
// where_entry_matches, so duplicates in the dictionary and repeated indices need no care.
//
// No atomics, no scratch buffer, every mask byte of a live column written exactly once: capturable as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_coop.h"
#include "covt_segscan.h"
#include "covt_select_plan.h"
#include "covt_wave.h"
#include "covt_where_plan.h"

namespace covt {

constexpr int kWhereWaves = 4;                // waves per workgroup
constexpr int kWhereCoopMaxColumns = 4096;    // batches of at most this many columns: a workgroup per column
// Dictionary entries a clause's LDS match bitmap covers.  8 clauses x 16,384 bits = 16 KiB a workgroup, which
// with the staged blob and the resolved clauses is 21 KiB: seven workgroups (28 of 32 waves) fit the 160 KiB of
// a CU, and the largest dictionary of the fixtures (8,925 entries) fits the bitmap.  A wave-per-column launch
// cuts the same 16 KiB four ways.
constexpr int kWhereDictBitsGroup = 16384;
constexpr int kWhereDictBitsWave = kWhereDictBitsGroup / kWhereWaves;
constexpr int kWhereDictPerFeature = 4;       // wave per column: bitmap while n_dict <= this * n_features
constexpr int kWhereBitmapWords = COVT_WHERE_MAX_CLAUSES * kWhereDictBitsGroup / 32;
static_assert(kWhereDictBitsWave % 64 == 0, "a wave stores its ballot as two whole words");

constexpr int32_t kWhereUnbound = -1;  // WhereCol::type of a clause without a column
constexpr int32_t kWhereNoType = 4;    // ... of a column whose type is none of COVT_PROP_*: nothing is defined

// clause k resolved for one geometry column
struct WhereCol {
    const uint8_t* validity;
    const uint8_t* values;
    const int32_t* doffs;
    const uint8_t* dbytes;
    int32_t op;
    uint32_t flags;
    int32_t first, count;  // its literals, inside covt_where.values
    int32_t type;          // COVT_PROP_*, kWhereUnbound, kWhereNoType
    int32_t n_dict, dict_bytes;
    int32_t bitmap;        // the clause is answered from the LDS match bitmap
    int32_t cause, pad;    // the column rule: COVT_OK or the status this clause gives the column
};

struct __attribute__((aligned(16))) WhereSmem {
    covt_where w;
    WhereCol col[kWhereWaves][COVT_WHERE_MAX_CLAUSES];
    uint32_t bits[kWhereBitmapWords];
};

// dictionary entry e (inside [0, n_dict)) equals one of the clause's string literals
__device__ __forceinline__ bool where_entry_matches(const covt_where& w, const WhereCol& q, int32_t e) {
    int32_t o, len;
    where_entry_range(((const g_i32*)q.doffs)[e], ((const g_i32*)q.doffs)[e + 1], q.dict_bytes, o, len);
    bool hit = false;
    for (int32_t j = 0; j < q.count && !hit; ++j) {
        const covt_where_value& L = w.values[q.first + j];
        int32_t so, sl;
        where_text_range(L.str_off, L.str_len, so, sl);
        if (!(L.kinds & COVT_WHERE_STRING) || sl != len) continue;
        int32_t i = 0;
        while (i < len && ((const g_u8*)q.dbytes)[o + i] == w.text[so + i]) ++i;
        hit = i == len;
    }
    return hit;
}

// truth of clause q for the features f .. f + 3 (f % 4 == 0, f < n), a bit each; bits past n are unspecified
__device__ __forceinline__ uint32_t where_clause_bits(const covt_where& w, const WhereCol& q, const uint32_t* bm,
                                                      int64_t f, int32_t n) {
    const uint32_t absent = where_absent_truth(q.op, q.flags) ? 0xfu : 0u;
    if (q.type == kWhereUnbound) return absent;
    const uint32_t valid = (uint32_t)(((const g_u8*)q.validity)[f >> 3] >> (f & 4)) & 0xfu;
    uint32_t eq = 0, lt = 0, gt = 0;
    if (q.op < COVT_WHERE_IS_NULL) {
        switch (q.type) {
        case COVT_PROP_BOOLEAN: {
            const uint32_t v = (uint32_t)(((const g_u8*)q.values)[f >> 3] >> (f & 4)) & 0xfu;
            for (int32_t j = 0; j < q.count; ++j) {
                const covt_where_value& L = w.values[q.first + j];
                if (L.kinds & COVT_WHERE_BOOL) eq |= L.b != 0 ? v : ~v;
            }
            break;
        }
        case COVT_PROP_INT64: {
            const g_u32x4* p = (const g_u32x4*)(q.values + 8 * f);
            const u32x4 a = p[0];
            u32x4 b = {0u, 0u, 0u, 0u};
            if (f + 2 < n) b = p[1];  // (a column of 4k + 1 or 4k + 2 features ends inside the first vector)
            const int64_t v[4] = {(int64_t)(((uint64_t)a.y << 32) | a.x), (int64_t)(((uint64_t)a.w << 32) | a.z),
                                  (int64_t)(((uint64_t)b.y << 32) | b.x), (int64_t)(((uint64_t)b.w << 32) | b.z)};
            for (int32_t j = 0; j < q.count; ++j) {
                const covt_where_value& L = w.values[q.first + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    eq |= where_eq_int(v[i], L) ? 1u << i : 0u;
                    if (j == 0) {
                        lt |= where_lt_int(v[i], L) ? 1u << i : 0u;
                        gt |= where_gt_int(v[i], L) ? 1u << i : 0u;
                    }
                }
            }
            break;
        }
        case COVT_PROP_FLOAT: {
            const u32x4 a = *(const g_u32x4*)(q.values + 4 * f);
            const float v[4] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
            for (int32_t j = 0; j < q.count; ++j) {
                const covt_where_value& L = w.values[q.first + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    eq |= where_eq_real(v[i], L) ? 1u << i : 0u;
                    if (j == 0) {
                        lt |= where_lt_real(v[i], L) ? 1u << i : 0u;
                        gt |= where_gt_real(v[i], L) ? 1u << i : 0u;
                    }
                }
            }
            break;
        }
        case COVT_PROP_STRING: {
            const u32x4 a = *(const g_u32x4*)(q.values + 4 * f);
            const uint32_t v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (v[i] >= (uint32_t)q.n_dict) continue;  // (an index outside the dictionary equals nothing)
                if (q.bitmap) eq |= ((bm[v[i] >> 5] >> (v[i] & 31u)) & 1u) << i;
                else if (((valid >> i) & 1u) && f + i < n) eq |= where_entry_matches(w, q, (int32_t)v[i]) ? 1u << i : 0u;
            }
            break;
        }
        default: break;
        }
    }
    const uint32_t present = where_present_bits(q.op, eq, lt, gt, 0xfu);
    return (valid & present) | (~valid & absent);
}

template <bool WAVE>
__global__ __launch_bounds__(64 * kWhereWaves) void where_kernel(
    const covt_prop_desc* __restrict__ pdescs, const uint8_t* __restrict__ props,
    const covt_prop_result* __restrict__ pres, int64_t n_props, const covt_select_desc* __restrict__ sdescs,
    int64_t n_cols, const covt_where* __restrict__ where, const int32_t* __restrict__ bind, int32_t mode,
    uint8_t* __restrict__ select, int32_t* __restrict__ status) {
    __shared__ WhereSmem sm;
    // the blob, once per workgroup
    for (uint32_t i = threadIdx.x; i < sizeof(covt_where) / 4; i += 64 * kWhereWaves)
        ((uint32_t*)&sm.w)[i] = ((const g_u32*)where)[i];
    __syncthreads();
    const int wv = uni((int32_t)(threadIdx.x >> 6));
    const int g = WAVE ? wv : 0;                              // the group's slot in LDS
    const int t = WAVE ? lane_id() : (int)threadIdx.x;        // the thread in its group
    auto group_sync = [&] {
        if (WAVE) wave_sync();
        else __syncthreads();
    };
    const int64_t col = WAVE ? uni64((int64_t)blockIdx.x * kWhereWaves + wv) : (int64_t)blockIdx.x;
    if (col >= n_cols) return;
    const bool first_group = WAVE || blockIdx.y == 0;  // (the one that reports the column's status)
    const covt_select_desc sd = sdescs[col];
    const int32_t n = sd.n_features;
    if ((sd.flags & COVT_SELECT_TOO_LARGE) || n <= 0) {
        if (status && first_group && t == 0) status[col] = COVT_OK;
        return;
    }
    const covt_where& w = sm.w;
    const int32_t nc = where_n_clauses(w.n_clauses);
    constexpr int32_t kBits = WAVE ? kWhereDictBitsWave : kWhereDictBitsGroup;
    uint32_t* const bits = sm.bits + (WAVE ? g * (kWhereBitmapWords / kWhereWaves) : 0);

    // ---- the clauses resolved for this column, thread k clause k --------------------------------------------
    if (t < nc) {
        const covt_where_clause c = w.clauses[t];
        WhereCol q{};
        q.op = c.op;
        q.flags = c.flags;
        where_value_range(c, q.first, q.count);
        q.type = kWhereUnbound;
        q.cause = COVT_OK;
        const int32_t b = bind[col * COVT_WHERE_MAX_CLAUSES + t];
        if (b < -1 || b >= n_props) {
            q.cause = COVT_ERR_INVALID_ARG;
        } else if (b >= 0) {
            const covt_prop_desc pd = pdescs[b];
            const int32_t st = pres[b].status;
            if (st != COVT_OK) {
                q.cause = st;
            } else if (pd.n_features != n) {
                q.cause = COVT_ERR_INVALID_ARG;
            } else {
                q.type = pd.type >= COVT_PROP_BOOLEAN && pd.type <= COVT_PROP_STRING ? pd.type : kWhereNoType;
                q.validity = props + pd.out_off[0];
                q.values = props + pd.out_off[1];
                if (q.type == COVT_PROP_STRING && pd.out_off[2] >= 0 && pd.out_off[3] >= 0) {  // (else: no dictionary)
                    q.doffs = (const int32_t*)(props + pd.out_off[2]);
                    q.dbytes = props + pd.out_off[3];
                    q.n_dict = max(pd.n_dict, 0);
                    q.dict_bytes = max(pd.dict_bytes, 0);
                }
                q.bitmap = q.type == COVT_PROP_STRING && q.op < COVT_WHERE_IS_NULL && q.count > 0 && q.n_dict > 0 &&
                           q.n_dict <= kBits && (!WAVE || (int64_t)q.n_dict <= (int64_t)kWhereDictPerFeature * n);
            }
        }
        sm.col[g][t] = q;
    }
    group_sync();
    const WhereCol* const cols = sm.col[g];

    // ---- the column rule: the lowest clause with a cause ----------------------------------------------------
    int32_t st = COVT_OK;
    for (int32_t k = nc - 1; k >= 0; --k)
        if (cols[k].cause != COVT_OK) st = cols[k].cause;
    if (status && first_group && t == 0) status[col] = st;

    uint8_t* const mask = select + sd.off + select_mask_off(n);
    const int64_t f0 = 4 * (WAVE ? (int64_t)t : (int64_t)blockIdx.y * (64 * kWhereWaves) + t);
    const int64_t step = 4 * (WAVE ? (int64_t)64 : (int64_t)gridDim.y * (64 * kWhereWaves));

    // ---- the match bitmaps of the string clauses -------------------------------------------------------------
    if (st == COVT_OK) {
        for (int32_t k = 0; k < nc; ++k) {
            const WhereCol& q = cols[k];
            if (!q.bitmap) continue;
            uint32_t* bm = bits + k * (kBits / 32);
            for (int32_t e0 = WAVE ? 0 : 64 * wv; e0 < q.n_dict; e0 += WAVE ? 64 : 64 * kWhereWaves) {
                const int32_t e = e0 + lane_id();
                const bool hit = e < q.n_dict && where_entry_matches(w, q, e);
                const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
                if (lane_id() == 0) {  // (e0 + 63 < kBits: n_dict <= kBits, a multiple of 64)
                    bm[e0 >> 5] = (uint32_t)m;
                    bm[(e0 >> 5) + 1] = (uint32_t)(m >> 32);
                }
            }
        }
        group_sync();
    }

    // ---- the features, four per lane ----------------------------------------------------------------------------
    for (int64_t f = f0; f < n; f += step) {
        uint32_t keep = st == COVT_OK ? 0xfu : 0u;
        if (st == COVT_OK)
            for (int32_t k = 0; k < nc; ++k) keep &= where_clause_bits(w, cols[k], bits + k * (kBits / 32), f, n);
        if (f + 4 <= n) {
            uint32_t old = 0x01010101u;
            if (mode == COVT_WHERE_AND) old = *(const g_u32*)(mask + f);
            uint32_t out = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                out |= (((keep >> i) & 1u) && ((old >> (8 * i)) & 0xffu)) ? 1u << (8 * i) : 0u;
            *(gw_u32*)(mask + f) = out;
        } else {
            for (int i = 0; f + i < n; ++i) {
                const bool old = mode == COVT_WHERE_AND ? ((const g_u8*)mask)[f + i] != 0 : true;
                ((gw_u8*)mask)[f + i] = (((keep >> i) & 1u) && old) ? 1 : 0;
            }
        }
    }
}

int where_launch(const covt_prop_desc* d_pdesc, const uint8_t* d_props, const covt_prop_result* d_pres, int64_t n_props,
                 const covt_select_desc* d_sdesc, int64_t n_columns, const covt_where* d_where, const int32_t* d_bind,
                 int32_t mode, uint8_t* d_select, int32_t* d_status, hipStream_t s) {
    if (n_columns <= kWhereCoopMaxColumns) {
        hipLaunchKernelGGL(where_kernel<false>, dim3((unsigned)n_columns, product_blocks_y(n_columns)),
                           dim3(64 * kWhereWaves), 0, s, d_pdesc, d_props, d_pres, n_props, d_sdesc, n_columns, d_where,
                           d_bind, mode, d_select, d_status);
    } else {
        hipLaunchKernelGGL(where_kernel<true>, dim3((unsigned)((n_columns + kWhereWaves - 1) / kWhereWaves)),
                           dim3(64 * kWhereWaves), 0, s, d_pdesc, d_props, d_pres, n_props, d_sdesc, n_columns, d_where,
                           d_bind, mode, d_select, d_status);
    }
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

}  // namespace covt

extern "C" void covt_where_init(covt_where* w) {
    if (w) where_init(w);
}

extern "C" int covt_where_add_clause(covt_where* w, const uint8_t* name, int32_t name_len, int32_t op, uint32_t flags,
                                     const covt_where_literal* literals, int32_t n) {
    return where_add_clause(w, name, name_len, op, flags, literals, n);
}

extern "C" int covt_where_valid(const covt_where* w) { return where_valid(w) ? 1 : 0; }

extern "C" int covt_where_bind(const covt_where* w, const covt_geom_info* ginfo, int64_t n_geom,
                               const covt_prop_info* pinfo, int64_t n_props, const uint8_t* bytes, uint64_t n_bytes,
                               int32_t* out) {
    return where_bind(w, ginfo, n_geom, pinfo, n_props, bytes, n_bytes, out);
}

extern "C" int32_t covt_where_dict_bound(int32_t which) {
    return which == 0 ? covt::kWhereDictBitsGroup : which == 1 ? covt::kWhereDictBitsWave : 0;
}

extern "C" int covt_select_where_device(const covt_prop_desc* d_pdesc, const uint8_t* d_props,
                                        const covt_prop_result* d_pres, int64_t n_prop_columns,
                                        const covt_select_desc* d_sdesc, int64_t n_columns, const covt_where* d_where,
                                        const int32_t* d_bind, int32_t mode, uint8_t* d_select, int32_t* d_status,
                                        void* hip_stream) {
    if (n_columns < 0 || n_prop_columns < 0 || (mode != COVT_WHERE_WRITE && mode != COVT_WHERE_AND))
        return COVT_ERR_INVALID_ARG;
    if (n_columns && (!d_sdesc || !d_where || !d_bind || !d_select || (n_prop_columns && (!d_pdesc || !d_props || !d_pres))))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff || n_prop_columns > 0x7fffffff || ((uintptr_t)d_select & 15) || ((uintptr_t)d_where & 7))
        return COVT_ERR_INVALID_ARG;
    return covt::where_launch(d_pdesc, d_props, d_pres, n_prop_columns, d_sdesc, n_columns, d_where, d_bind, mode,
                              d_select, d_status, (hipStream_t)hip_stream);
}

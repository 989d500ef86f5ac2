// covt_where_plan.h -- the property predicate's rules (include/covt.h "Property predicates"), shared by the host
// entry points (covt_where.hip, covt_host.cpp) and the kernel (covt_where.hip): the blob's argument rule, the
// clamps the kernel reads it with, the single-value comparisons, and on the host the clause builder and the bind
// rule.  Plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_WHERE_PLAN_H
#define COVT_WHERE_PLAN_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_WHERE_HD __host__ __device__
#else
#define COVT_WHERE_HD
#endif

constexpr uint32_t kWhereKinds = COVT_WHERE_BOOL | COVT_WHERE_INT | COVT_WHERE_REAL | COVT_WHERE_STRING;

COVT_WHERE_HD inline int32_t where_clamp(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : x > hi ? hi : x; }

// ---- the argument rule ---------------------------------------------------------------------------------
COVT_WHERE_HD inline bool where_op_valid(int32_t op) { return op >= COVT_WHERE_EQ && op <= COVT_WHERE_NOT_NULL; }
// values a clause of `op` takes: [lo, hi]
COVT_WHERE_HD inline void where_op_values(int32_t op, int32_t& lo, int32_t& hi) {
    if (op == COVT_WHERE_IS_NULL || op == COVT_WHERE_NOT_NULL) lo = hi = 0;
    else if (op == COVT_WHERE_IN || op == COVT_WHERE_NOT_IN) lo = 1, hi = COVT_WHERE_MAX_IN;
    else lo = hi = 1;
}
COVT_WHERE_HD inline bool where_value_valid(const covt_where_value& v, uint32_t text_len) {
    if (!(v.kinds & kWhereKinds) || (v.kinds & ~kWhereKinds) || v.d != v.d) return false;
    return v.str_off >= 0 && v.str_len >= 0 && (uint32_t)v.str_off <= text_len &&
           (uint32_t)v.str_len <= text_len - (uint32_t)v.str_off;
}
// the blob covt_where_add_clause builds: its size, counts inside the arrays, every clause's op, flags, value
// count and ranges, every value's kinds, no NaN
COVT_WHERE_HD inline bool where_valid(const covt_where* w) {
    if (!w || w->size != (uint32_t)sizeof(covt_where)) return false;
    if (w->n_clauses > COVT_WHERE_MAX_CLAUSES || w->n_values > COVT_WHERE_MAX_VALUES || w->text_len > COVT_WHERE_MAX_TEXT)
        return false;
    for (uint32_t k = 0; k < w->n_clauses; ++k) {
        const covt_where_clause& c = w->clauses[k];
        if (!where_op_valid(c.op) || (c.flags & ~(uint32_t)COVT_WHERE_NULL_MATCHES)) return false;
        int32_t lo, hi;
        where_op_values(c.op, lo, hi);
        if (c.n_values < lo || c.n_values > hi || c.first_value < 0 || (uint32_t)c.first_value > w->n_values ||
            (uint32_t)c.n_values > w->n_values - (uint32_t)c.first_value)
            return false;
        if (c.name_off < 0 || c.name_len < 0 || (uint32_t)c.name_off > w->text_len ||
            (uint32_t)c.name_len > w->text_len - (uint32_t)c.name_off)
            return false;
    }
    for (uint32_t j = 0; j < w->n_values; ++j)
        if (!where_value_valid(w->values[j], w->text_len)) return false;
    return true;
}

// ---- the blob as the kernel reads it: every count and range clamped to the blob's own arrays ------------
COVT_WHERE_HD inline int32_t where_n_clauses(uint32_t n_clauses) {
    return n_clauses > COVT_WHERE_MAX_CLAUSES ? COVT_WHERE_MAX_CLAUSES : (int32_t)n_clauses;
}
COVT_WHERE_HD inline void where_value_range(const covt_where_clause& c, int32_t& first, int32_t& count) {
    first = where_clamp(c.first_value, 0, COVT_WHERE_MAX_VALUES);
    count = where_clamp(c.n_values, 0, COVT_WHERE_MAX_VALUES - first);
}
COVT_WHERE_HD inline void where_text_range(int32_t off, int32_t len, int32_t& o, int32_t& n) {
    o = where_clamp(off, 0, COVT_WHERE_MAX_TEXT);
    n = where_clamp(len, 0, COVT_WHERE_MAX_TEXT - o);
}

// ---- the comparisons -----------------------------------------------------------------------------------
// eq / lt / gt of one value against one literal; false where the literal lacks the column's kind
COVT_WHERE_HD inline bool where_eq_bool(bool v, const covt_where_value& L) {
    return (L.kinds & COVT_WHERE_BOOL) && v == (L.b != 0);
}
COVT_WHERE_HD inline bool where_eq_int(int64_t v, const covt_where_value& L) { return (L.kinds & COVT_WHERE_INT) && v == L.i; }
COVT_WHERE_HD inline bool where_lt_int(int64_t v, const covt_where_value& L) { return (L.kinds & COVT_WHERE_INT) && v < L.i; }
COVT_WHERE_HD inline bool where_gt_int(int64_t v, const covt_where_value& L) { return (L.kinds & COVT_WHERE_INT) && v > L.i; }
COVT_WHERE_HD inline bool where_eq_real(float v, const covt_where_value& L) {
    return (L.kinds & COVT_WHERE_REAL) && (double)v == L.d;
}
COVT_WHERE_HD inline bool where_lt_real(float v, const covt_where_value& L) {
    return (L.kinds & COVT_WHERE_REAL) && (double)v < L.d;
}
COVT_WHERE_HD inline bool where_gt_real(float v, const covt_where_value& L) {
    return (L.kinds & COVT_WHERE_REAL) && (double)v > L.d;
}
// a dictionary entry's bytes [o, o + n) from dict_offsets[v], [v + 1], read clamped to [0, dict_bytes]
COVT_WHERE_HD inline void where_entry_range(int32_t off0, int32_t off1, int32_t dict_bytes, int32_t& o, int32_t& n) {
    o = where_clamp(off0, 0, dict_bytes);
    const int32_t e = where_clamp(off1, 0, dict_bytes);
    n = e > o ? e - o : 0;
}
COVT_WHERE_HD inline bool where_eq_bytes(const uint8_t* a, const uint8_t* b, int32_t n) {
    for (int32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}
// present values' truth under `op`, a bit per value (`all`: the bits in use): eq = some literal equal (EQ / NE:
// the one literal), lt / gt against the first literal
COVT_WHERE_HD inline uint32_t where_present_bits(int32_t op, uint32_t eq, uint32_t lt, uint32_t gt, uint32_t all) {
    switch (op) {
    case COVT_WHERE_EQ:
    case COVT_WHERE_IN: return eq & all;
    case COVT_WHERE_NE:
    case COVT_WHERE_NOT_IN: return ~eq & all;
    case COVT_WHERE_LT: return lt & all;
    case COVT_WHERE_LE: return (lt | eq) & all;
    case COVT_WHERE_GT: return gt & all;
    case COVT_WHERE_GE: return (gt | eq) & all;
    case COVT_WHERE_NOT_NULL: return all;
    default: return 0u;  // IS_NULL, and an op no valid blob holds
    }
}
COVT_WHERE_HD inline bool where_present_truth(int32_t op, bool eq, bool lt, bool gt) {
    return where_present_bits(op, eq ? 1u : 0u, lt ? 1u : 0u, gt ? 1u : 0u, 1u) != 0;
}
COVT_WHERE_HD inline bool where_absent_truth(int32_t op, uint32_t flags) {
    if (op == COVT_WHERE_IS_NULL) return true;
    if (op == COVT_WHERE_NOT_NULL) return false;
    return (flags & COVT_WHERE_NULL_MATCHES) != 0;
}

// One present value of a column of `type` (COVT_PROP_*) against clause c of blob w: the definition in one
// place, value by value.  The value: BOOLEAN vb, INT64 vi, FLOAT vf, STRING the entry's bytes (entry null: an
// index outside the dictionary).
COVT_WHERE_HD inline bool where_clause_present(const covt_where& w, const covt_where_clause& c, int32_t type, bool vb,
                                               int64_t vi, float vf, const uint8_t* entry, int32_t entry_len) {
    int32_t first, count;
    where_value_range(c, first, count);
    bool eq = false, lt = false, gt = false;
    for (int32_t j = 0; j < count; ++j) {
        const covt_where_value& L = w.values[first + j];
        switch (type) {
        case COVT_PROP_BOOLEAN: eq = eq || where_eq_bool(vb, L); break;
        case COVT_PROP_INT64:
            eq = eq || where_eq_int(vi, L);
            if (j == 0) lt = where_lt_int(vi, L), gt = where_gt_int(vi, L);
            break;
        case COVT_PROP_FLOAT:
            eq = eq || where_eq_real(vf, L);
            if (j == 0) lt = where_lt_real(vf, L), gt = where_gt_real(vf, L);
            break;
        case COVT_PROP_STRING: {
            int32_t so, sl;
            where_text_range(L.str_off, L.str_len, so, sl);
            eq = eq || ((L.kinds & COVT_WHERE_STRING) && entry && sl == entry_len && where_eq_bytes(entry, w.text + so, sl));
            break;
        }
        default: break;
        }
    }
    return where_present_truth(c.op, eq, lt, gt);
}

// ---- host only: the clause builder and the bind rule ------------------------------------------------------
inline void where_init(covt_where* w) {
    memset(w, 0, sizeof(*w));
    w->size = (uint32_t)sizeof(covt_where);
}

// one more clause, or COVT_ERR_INVALID_ARG with *w untouched
inline int where_add_clause(covt_where* w, const uint8_t* name, int32_t name_len, int32_t op, uint32_t flags,
                            const covt_where_literal* lits, int32_t n) {
    if (!where_valid(w) || name_len < 0 || (!name && name_len) || !where_op_valid(op) ||
        (flags & ~(uint32_t)COVT_WHERE_NULL_MATCHES) || n < 0 || (!lits && n))
        return COVT_ERR_INVALID_ARG;
    int32_t lo, hi;
    where_op_values(op, lo, hi);
    if (n < lo || n > hi || w->n_clauses >= COVT_WHERE_MAX_CLAUSES || (uint32_t)n > COVT_WHERE_MAX_VALUES - w->n_values)
        return COVT_ERR_INVALID_ARG;
    uint64_t text = (uint64_t)w->text_len + (uint64_t)name_len;
    for (int32_t j = 0; j < n; ++j) {
        const covt_where_literal& L = lits[j];
        if (!(L.kinds & kWhereKinds) || (L.kinds & ~kWhereKinds) || L.d != L.d) return COVT_ERR_INVALID_ARG;
        if (L.kinds & COVT_WHERE_STRING) {
            if (L.str_len < 0 || (!L.str && L.str_len)) return COVT_ERR_INVALID_ARG;
            text += (uint64_t)L.str_len;
        }
    }
    if (text > COVT_WHERE_MAX_TEXT) return COVT_ERR_INVALID_ARG;
    // (nothing fails from here on)
    covt_where_clause& c = w->clauses[w->n_clauses++];
    memset(&c, 0, sizeof(c));
    c.op = op;
    c.flags = flags;
    c.first_value = (int32_t)w->n_values;
    c.n_values = n;
    c.name_off = (int32_t)w->text_len;
    c.name_len = name_len;
    if (name_len) memcpy(w->text + w->text_len, name, (size_t)name_len);
    w->text_len += (uint32_t)name_len;
    for (int32_t j = 0; j < n; ++j) {
        const covt_where_literal& L = lits[j];
        covt_where_value& v = w->values[w->n_values++];
        memset(&v, 0, sizeof(v));
        v.kinds = L.kinds;
        v.b = L.b;
        v.i = L.i;
        v.d = L.d;
        if (L.kinds & COVT_WHERE_STRING) {
            v.str_off = (int32_t)w->text_len;
            v.str_len = L.str_len;
            if (L.str_len) memcpy(w->text + w->text_len, L.str, (size_t)L.str_len);
            w->text_len += (uint32_t)L.str_len;
        }
    }
    return COVT_OK;
}

// a property record's full name (column name, plus ':' + language of a localized sub-column) equals name[0, n)
inline bool where_name_matches(const covt_prop_info& p, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* name,
                               int32_t n) {
    auto inside = [&](int64_t off, int32_t len) {
        return len >= 0 && off >= 0 && (uint64_t)off <= n_bytes && (uint64_t)len <= n_bytes - (uint64_t)off;
    };
    // (a record without a column name is spelled "")
    const int32_t nl = p.name_off >= 0 ? p.name_len : 0;
    if (p.name_off >= 0 && !inside(p.name_off, p.name_len)) return false;
    if (p.lang < 0) return nl == n && (n == 0 || memcmp(bytes + p.name_off, name, (size_t)n) == 0);
    if (!inside(p.lang_off, p.lang_len)) return false;
    if ((int64_t)nl + 1 + p.lang_len != n) return false;
    if (nl && memcmp(bytes + p.name_off, name, (size_t)nl) != 0) return false;
    if (name[nl] != ':') return false;
    return p.lang_len == 0 || memcmp(bytes + p.lang_off, name + nl + 1, (size_t)p.lang_len) == 0;
}

// out[g.desc_index * COVT_WHERE_MAX_CLAUSES + k]: the desc_index of the first property record, in tile order,
// of g's tile and layer whose full name is clause k's; -1 without one and for the unused clause slots
inline int where_bind(const covt_where* w, const covt_geom_info* ginfo, int64_t n_geom, const covt_prop_info* pinfo,
                      int64_t n_props, const uint8_t* bytes, uint64_t n_bytes, int32_t* out) {
    if (!where_valid(w) || n_geom < 0 || n_props < 0 || (n_geom && (!ginfo || !out)) || (n_props && !pinfo) ||
        (!bytes && n_bytes))
        return COVT_ERR_INVALID_ARG;
    for (int64_t c = 0; c < n_geom; ++c)
        if (ginfo[c].desc_index < 0 || ginfo[c].desc_index >= n_geom) return COVT_ERR_INVALID_ARG;
    // the records of one (tile, layer) through an index sorted by that pair (stable: tile order inside it)
    auto key_less = [&](int64_t a, int64_t b) {
        return pinfo[a].tile != pinfo[b].tile ? pinfo[a].tile < pinfo[b].tile : pinfo[a].layer < pinfo[b].layer;
    };
    std::vector<int64_t> order((size_t)n_props);
    for (int64_t i = 0; i < n_props; ++i) order[(size_t)i] = i;
    if (!std::is_sorted(order.begin(), order.end(), key_less)) std::stable_sort(order.begin(), order.end(), key_less);
    for (int64_t c = 0; c < n_geom; ++c) {
        const covt_geom_info& g = ginfo[c];
        int32_t* row = out + (int64_t)g.desc_index * COVT_WHERE_MAX_CLAUSES;
        for (int k = 0; k < COVT_WHERE_MAX_CLAUSES; ++k) row[k] = -1;
        auto lo = std::partition_point(order.begin(), order.end(), [&](int64_t i) {
            return pinfo[i].tile != g.tile ? pinfo[i].tile < g.tile : pinfo[i].layer < g.layer;
        });
        for (uint32_t k = 0; k < w->n_clauses; ++k) {
            const covt_where_clause& cl = w->clauses[k];
            for (auto it = lo; it != order.end() && pinfo[*it].tile == g.tile && pinfo[*it].layer == g.layer; ++it)
                if (where_name_matches(pinfo[*it], bytes, n_bytes, w->text + cl.name_off, cl.name_len)) {
                    row[k] = pinfo[*it].desc_index;
                    break;
                }
        }
    }
    return COVT_OK;
}

#endif

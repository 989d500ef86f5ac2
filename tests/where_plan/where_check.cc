// where_check.cc -- covt_where_plan.h on the CPU, built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_where_ref.py: the blob's argument rule (and that a refused clause leaves the blob untouched), the
// single-value comparison of every column type against a table written out here, and the bind rule on hand-made
// records.  Prints "ok" and the number of checks.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "covt_where_plan.h"

static long g_checks = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        ++g_checks;                                                     \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static covt_where_literal L_bool(bool b) { return covt_where_literal{COVT_WHERE_BOOL, b ? 1 : 0, 0, 0.0, nullptr, 0, 0}; }
static covt_where_literal L_int(int64_t i) { return covt_where_literal{COVT_WHERE_INT, 0, i, 0.0, nullptr, 0, 0}; }
static covt_where_literal L_real(double d) { return covt_where_literal{COVT_WHERE_REAL, 0, 0, d, nullptr, 0, 0}; }
static covt_where_literal L_num(int64_t i) {
    return covt_where_literal{COVT_WHERE_INT | COVT_WHERE_REAL, 0, i, (double)i, nullptr, 0, 0};
}
static covt_where_literal L_str(const char* s) {
    return covt_where_literal{COVT_WHERE_STRING, 0, 0, 0.0, (const uint8_t*)s, (int32_t)strlen(s), 0};
}
static int add(covt_where* w, const char* name, int32_t op, uint32_t flags, std::vector<covt_where_literal> lits) {
    return where_add_clause(w, (const uint8_t*)name, (int32_t)strlen(name), op, flags, lits.data(), (int32_t)lits.size());
}
// the add is refused and the blob is byte for byte what it was
static void refused(covt_where* w, const char* name, int32_t op, uint32_t flags, std::vector<covt_where_literal> lits) {
    covt_where before;
    memcpy(&before, w, sizeof(before));
    CHECK(add(w, name, op, flags, lits) == COVT_ERR_INVALID_ARG);
    CHECK(memcmp(&before, w, sizeof(before)) == 0);
}

static void check_validation() {
    CHECK(sizeof(covt_where_value) == 32 && sizeof(covt_where_clause) == 32 && sizeof(covt_where) == 2320);
    covt_where w;
    memset(&w, 0xEE, sizeof(w));
    CHECK(!where_valid(&w) && !where_valid(nullptr));
    where_init(&w);
    CHECK(where_valid(&w) && w.size == 2320 && w.n_clauses == 0 && w.n_values == 0 && w.text_len == 0);
    // the value counts of every op
    for (int op = COVT_WHERE_EQ; op <= COVT_WHERE_NOT_NULL; ++op) {
        int32_t lo, hi;
        where_op_values(op, lo, hi);
        for (int n = 0; n <= COVT_WHERE_MAX_IN + 1; ++n) {
            covt_where x;
            where_init(&x);
            std::vector<covt_where_literal> lits((size_t)n, L_int(7));
            const int st = add(&x, "c", op, 0, lits);
            CHECK((st == COVT_OK) == (n >= lo && n <= hi));
            CHECK(where_valid(&x) && x.n_clauses == (st == COVT_OK ? 1u : 0u));
        }
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    refused(&w, "c", -1, 0, {L_int(1)});
    refused(&w, "c", 10, 0, {L_int(1)});
    refused(&w, "c", COVT_WHERE_EQ, 2, {L_int(1)});
    refused(&w, "c", COVT_WHERE_EQ, 0, {covt_where_literal{0, 0, 1, 1.0, nullptr, 0, 0}});    // no kind bit
    refused(&w, "c", COVT_WHERE_EQ, 0, {covt_where_literal{16, 0, 1, 1.0, nullptr, 0, 0}});   // an unknown one
    refused(&w, "c", COVT_WHERE_EQ, 0, {L_real(nan)});
    refused(&w, "c", COVT_WHERE_IN, 0, {L_int(1), covt_where_literal{COVT_WHERE_INT, 0, 1, nan, nullptr, 0, 0}});
    refused(&w, "c", COVT_WHERE_EQ, 0, {covt_where_literal{COVT_WHERE_STRING, 0, 0, 0.0, nullptr, 3, 0}});
    refused(&w, "c", COVT_WHERE_EQ, 0, {covt_where_literal{COVT_WHERE_STRING, 0, 0, 0.0, (const uint8_t*)"x", -1, 0}});
    CHECK(where_add_clause(&w, nullptr, 1, COVT_WHERE_IS_NULL, 0, nullptr, 0) == COVT_ERR_INVALID_ARG);
    CHECK(where_add_clause(&w, (const uint8_t*)"c", -1, COVT_WHERE_IS_NULL, 0, nullptr, 0) == COVT_ERR_INVALID_ARG);
    CHECK(where_add_clause(&w, (const uint8_t*)"c", 1, COVT_WHERE_EQ, 0, nullptr, 1) == COVT_ERR_INVALID_ARG);
    CHECK(where_add_clause(nullptr, (const uint8_t*)"c", 1, COVT_WHERE_IS_NULL, 0, nullptr, 0) == COVT_ERR_INVALID_ARG);
    // the layout: per clause its name, then its string literals
    CHECK(add(&w, "class", COVT_WHERE_IN, 0, {L_str("motorway"), L_num(3), L_str("")}) == COVT_OK);
    CHECK(add(&w, "", COVT_WHERE_IS_NULL, COVT_WHERE_NULL_MATCHES, {}) == COVT_OK);
    CHECK(w.n_clauses == 2 && w.n_values == 3 && w.text_len == 13 && memcmp(w.text, "classmotorway", 13) == 0);
    CHECK(w.clauses[0].name_off == 0 && w.clauses[0].name_len == 5 && w.clauses[0].first_value == 0 && w.clauses[0].n_values == 3);
    CHECK(w.values[0].str_off == 5 && w.values[0].str_len == 8 && w.values[0].kinds == COVT_WHERE_STRING);
    CHECK(w.values[1].kinds == 6 && w.values[1].i == 3 && w.values[1].d == 3.0 && w.values[1].str_len == 0);
    CHECK(w.values[2].str_off == 13 && w.values[2].str_len == 0);
    CHECK(w.clauses[1].name_off == 13 && w.clauses[1].name_len == 0 && w.clauses[1].first_value == 3 && w.clauses[1].flags == 1);
    CHECK(where_valid(&w));
    // a ninth clause
    covt_where c8;
    where_init(&c8);
    for (int k = 0; k < 8; ++k) CHECK(add(&c8, "n", COVT_WHERE_NOT_NULL, 0, {}) == COVT_OK);
    refused(&c8, "n", COVT_WHERE_NOT_NULL, 0, {});
    // a 33rd value
    covt_where v32;
    where_init(&v32);
    CHECK(add(&v32, "a", COVT_WHERE_IN, 0, std::vector<covt_where_literal>(16, L_int(1))) == COVT_OK);
    CHECK(add(&v32, "b", COVT_WHERE_IN, 0, std::vector<covt_where_literal>(15, L_int(1))) == COVT_OK);
    refused(&v32, "c", COVT_WHERE_IN, 0, {L_int(1), L_int(2)});
    CHECK(add(&v32, "c", COVT_WHERE_EQ, 0, {L_int(1)}) == COVT_OK && v32.n_values == 32);
    refused(&v32, "d", COVT_WHERE_EQ, 0, {L_int(1)});
    CHECK(add(&v32, "d", COVT_WHERE_IS_NULL, 0, {}) == COVT_OK);
    // text past 1024 bytes: 1024 fit, 1025 do not
    const std::string s500(500, 'x'), s519(519, 'y'), s520(520, 'z');
    covt_where t;
    where_init(&t);
    CHECK(add(&t, "name", COVT_WHERE_EQ, 0, {L_str(s500.c_str())}) == COVT_OK && t.text_len == 504);
    refused(&t, "n", COVT_WHERE_EQ, 0, {L_str(s520.c_str())});
    CHECK(add(&t, "n", COVT_WHERE_EQ, 0, {L_str(s519.c_str())}) == COVT_OK && t.text_len == 1024 && where_valid(&t));
    refused(&t, "n", COVT_WHERE_IS_NULL, 0, {});
    CHECK(add(&t, "", COVT_WHERE_IS_NULL, 0, {}) == COVT_OK);
    // blobs no add builds
    covt_where bad = w;
    bad.size = 2319;
    CHECK(!where_valid(&bad));
    bad = w, bad.n_clauses = 9;
    CHECK(!where_valid(&bad));
    bad = w, bad.clauses[0].first_value = 1;
    CHECK(!where_valid(&bad));
    bad = w, bad.clauses[0].name_len = 14;
    CHECK(!where_valid(&bad));
    bad = w, bad.values[0].str_off = 6;
    CHECK(!where_valid(&bad));
    bad = w, bad.values[1].d = nan;
    CHECK(!where_valid(&bad));
    bad = w, bad.values[1].kinds = 0;
    CHECK(!where_valid(&bad));
    // the kernel's clamps stay inside the arrays whatever the fields hold
    const int32_t wild[] = {INT32_MIN, -1, 0, 1, 31, 32, 33, 1023, 1024, 1025, INT32_MAX};
    for (int32_t a : wild)
        for (int32_t b : wild) {
            covt_where_clause c{};
            c.first_value = a, c.n_values = b;
            int32_t f, n;
            where_value_range(c, f, n);
            CHECK(f >= 0 && n >= 0 && f + n <= COVT_WHERE_MAX_VALUES);
            where_text_range(a, b, f, n);
            CHECK(f >= 0 && n >= 0 && f + n <= COVT_WHERE_MAX_TEXT);
            where_entry_range(a, b, 1000, f, n);
            CHECK(f >= 0 && n >= 0 && f + n <= 1000);
        }
    CHECK(where_n_clauses(0) == 0 && where_n_clauses(8) == 8 && where_n_clauses(9) == 8 && where_n_clauses(0xffffffffu) == 8);
}

// one clause over one present value
static bool truth(int32_t op, std::vector<covt_where_literal> lits, int32_t type, bool vb, int64_t vi, float vf,
                  const char* entry) {
    covt_where w;
    where_init(&w);
    CHECK(add(&w, "c", op, 0, lits) == COVT_OK);
    return where_clause_present(w, w.clauses[0], type, vb, vi, vf, (const uint8_t*)entry, entry ? (int32_t)strlen(entry) : 0);
}

static void check_compare() {
    const int64_t I64MIN = std::numeric_limits<int64_t>::min(), I64MAX = std::numeric_limits<int64_t>::max();
    const float inf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
    const int B = COVT_PROP_BOOLEAN, I = COVT_PROP_INT64, F = COVT_PROP_FLOAT, S = COVT_PROP_STRING;
    // {op, value, literal} -> truth, INT64: EQ NE LT LE GT GE
    struct { int64_t v, l; bool t[6]; } ints[] = {
        {0, 0, {true, false, false, true, false, true}},    {-1, 0, {false, true, true, true, false, false}},
        {1, 0, {false, true, false, false, true, true}},    {I64MIN, I64MIN, {true, false, false, true, false, true}},
        {I64MIN, I64MAX, {false, true, true, true, false, false}}, {I64MAX, I64MIN, {false, true, false, false, true, true}},
        {I64MAX, I64MAX, {true, false, false, true, false, true}}, {I64MAX - 1, I64MAX, {false, true, true, true, false, false}},
    };
    for (auto& r : ints)
        for (int op = 0; op < 6; ++op) CHECK(truth(op, {L_int(r.l)}, I, false, r.v, 0.f, nullptr) == r.t[op]);
    struct { float v; double l; bool t[6]; } reals[] = {
        {0.f, 0.0, {true, false, false, true, false, true}},    {-0.f, 0.0, {true, false, false, true, false, true}},
        {0.1f, 0.1, {false, true, false, false, true, true}},   {0.1f, (double)0.1f, {true, false, false, true, false, true}},
        {fnan, 0.0, {false, true, false, false, false, false}}, {inf, 1e308, {false, true, false, false, true, true}},
        {-inf, -1e308, {false, true, true, true, false, false}}, {1e-45f, 0.0, {false, true, false, false, true, true}},
        {inf, (double)inf, {true, false, false, true, false, true}},
    };
    for (auto& r : reals)
        for (int op = 0; op < 6; ++op) CHECK(truth(op, {L_real(r.l)}, F, false, 0, r.v, nullptr) == r.t[op]);
    // BOOLEAN: equality only
    for (int v = 0; v < 2; ++v)
        for (int l = 0; l < 2; ++l) {
            CHECK(truth(COVT_WHERE_EQ, {L_bool(l)}, B, v, 0, 0.f, nullptr) == (v == l));
            CHECK(truth(COVT_WHERE_NE, {L_bool(l)}, B, v, 0, 0.f, nullptr) == (v != l));
            for (int op = COVT_WHERE_LT; op <= COVT_WHERE_GE; ++op)
                CHECK(truth(op, {L_bool(l)}, B, v, 0, 0.f, nullptr) == ((op == COVT_WHERE_LE || op == COVT_WHERE_GE) && v == l));
        }
    CHECK(truth(COVT_WHERE_EQ, {covt_where_literal{COVT_WHERE_BOOL, 0x100, 0, 0.0, nullptr, 0, 0}}, B, true, 0, 0.f, nullptr));
    // STRING: lengths, then bytes; an index outside the dictionary (no entry) equals nothing
    CHECK(truth(COVT_WHERE_EQ, {L_str("trunk")}, S, false, 0, 0.f, "trunk"));
    CHECK(!truth(COVT_WHERE_EQ, {L_str("trunk")}, S, false, 0, 0.f, "trunk_link"));
    CHECK(!truth(COVT_WHERE_EQ, {L_str("trunk_link")}, S, false, 0, 0.f, "trunk"));
    CHECK(!truth(COVT_WHERE_EQ, {L_str("trunk")}, S, false, 0, 0.f, "trunK"));
    CHECK(truth(COVT_WHERE_EQ, {L_str("")}, S, false, 0, 0.f, ""));
    CHECK(!truth(COVT_WHERE_EQ, {L_str("")}, S, false, 0, 0.f, nullptr));
    CHECK(truth(COVT_WHERE_NE, {L_str("")}, S, false, 0, 0.f, nullptr));
    CHECK(truth(COVT_WHERE_IN, {L_str("a"), L_str("bb"), L_str("trunk")}, S, false, 0, 0.f, "trunk"));
    CHECK(truth(COVT_WHERE_NOT_IN, {L_str("a"), L_str("bb")}, S, false, 0, 0.f, "trunk"));
    for (int op = COVT_WHERE_LT; op <= COVT_WHERE_GE; ++op)
        CHECK(truth(op, {L_str("b")}, S, false, 0, 0.f, "a") == false && truth(op, {L_str("a")}, S, false, 0, 0.f, "a") ==
                                                                             (op == COVT_WHERE_LE || op == COVT_WHERE_GE));
    // kinds: a literal compares only with a column of one of its kinds
    CHECK(!truth(COVT_WHERE_EQ, {L_int(1)}, F, false, 0, 1.f, nullptr) && truth(COVT_WHERE_NE, {L_int(1)}, F, false, 0, 1.f, nullptr));
    CHECK(!truth(COVT_WHERE_LE, {L_int(1)}, F, false, 0, 1.f, nullptr) && !truth(COVT_WHERE_GE, {L_int(1)}, F, false, 0, 1.f, nullptr));
    CHECK(!truth(COVT_WHERE_EQ, {L_real(1.0)}, I, false, 1, 0.f, nullptr) && !truth(COVT_WHERE_LT, {L_real(2.0)}, I, false, 1, 0.f, nullptr));
    CHECK(truth(COVT_WHERE_EQ, {L_num(1)}, I, false, 1, 0.f, nullptr) && truth(COVT_WHERE_EQ, {L_num(1)}, F, false, 0, 1.f, nullptr));
    CHECK(!truth(COVT_WHERE_EQ, {L_num(1)}, B, true, 0, 0.f, nullptr) && !truth(COVT_WHERE_EQ, {L_num(1)}, S, false, 0, 0.f, "1"));
    CHECK(!truth(COVT_WHERE_EQ, {L_str("1")}, I, false, 1, 0.f, nullptr) && !truth(COVT_WHERE_EQ, {L_bool(true)}, I, false, 1, 0.f, nullptr));
    CHECK(truth(COVT_WHERE_IN, {L_str("x"), L_real(0.5), L_int(4)}, I, false, 4, 0.f, nullptr));
    CHECK(!truth(COVT_WHERE_IN, {L_str("x"), L_real(4.0)}, I, false, 4, 0.f, nullptr));
    // null ops and the absent rule
    for (int ty : {B, I, F, S}) {
        CHECK(!truth(COVT_WHERE_IS_NULL, {}, ty, false, 0, 0.f, "") && truth(COVT_WHERE_NOT_NULL, {}, ty, false, 0, 0.f, ""));
    }
    for (int op = 0; op <= COVT_WHERE_NOT_NULL; ++op) {
        CHECK(where_absent_truth(op, 0) == (op == COVT_WHERE_IS_NULL));
        CHECK(where_absent_truth(op, COVT_WHERE_NULL_MATCHES) == (op != COVT_WHERE_NOT_NULL));
    }
}

static void check_bind() {
    //                    0         1         2         3
    //                    0123456789012345678901234567890123456789
    const char* bytes = "classnamedeenrankclass";
    const uint64_t nb = strlen(bytes);
    auto prop = [](int32_t tile, int32_t layer, int64_t name_off, int32_t name_len, int32_t lang, int64_t lang_off,
                   int32_t lang_len, int32_t desc) {
        covt_prop_info p{};
        p.tile = tile, p.layer = layer, p.name_off = name_off, p.name_len = name_len, p.lang = lang;
        p.lang_off = lang_off, p.lang_len = lang_len, p.desc_index = desc;
        return p;
    };
    std::vector<covt_prop_info> pinfo = {
        prop(0, 0, 0, 5, -1, -1, 0, 7),    // tile 0 layer 0: class
        prop(0, 0, 5, 4, 0, 9, 2, 3),      //   name:de
        prop(0, 0, 5, 4, 1, 11, 2, 4),     //   name:en
        prop(0, 0, 17, 5, -1, -1, 0, 1),   //   class again: the first one wins
        prop(0, 1, 13, 4, -1, -1, 0, 0),   // tile 0 layer 1: rank
        prop(0, 1, 5, 4, -1, -1, 0, 8),    //   name (no language)
        prop(1, 0, 13, 4, -1, -1, 0, 5),   // tile 1 layer 0: rank
        prop(1, 0, 18, 5, -1, -1, 0, 2),   //   a name that leaves the bytes
        prop(1, 0, 5, 4, 0, 21, 2, 6),     //   a language that leaves the bytes
        prop(1, 0, -1, 0, -1, -1, 0, 9),   //   a record without a name: ""
    };
    auto geom = [](int32_t tile, int32_t layer, int32_t desc) {
        covt_geom_info g{};
        g.tile = tile, g.layer = layer, g.desc_index = desc;
        return g;
    };
    std::vector<covt_geom_info> ginfo = {geom(0, 0, 2), geom(0, 1, 0), geom(1, 0, 3), geom(1, 1, 1)};
    covt_where w;
    where_init(&w);
    CHECK(add(&w, "class", COVT_WHERE_IN, 0, {L_str("motorway")}) == COVT_OK);
    CHECK(add(&w, "rank", COVT_WHERE_LE, 0, {L_num(3)}) == COVT_OK);
    CHECK(add(&w, "name:de", COVT_WHERE_IS_NULL, 0, {}) == COVT_OK);
    CHECK(add(&w, "name", COVT_WHERE_NOT_NULL, 0, {}) == COVT_OK);
    CHECK(add(&w, "", COVT_WHERE_NOT_NULL, 0, {}) == COVT_OK);
    CHECK(add(&w, "name:", COVT_WHERE_NOT_NULL, 0, {}) == COVT_OK);
    std::vector<int32_t> out(4 * 8, 77);
    CHECK(where_bind(&w, ginfo.data(), 4, pinfo.data(), (int64_t)pinfo.size(), (const uint8_t*)bytes, nb, out.data()) == COVT_OK);
    const int32_t want[4][8] = {
        {-1, 0, -1, 8, -1, -1, -1, -1},   // descriptor 0: tile 0 layer 1
        {-1, -1, -1, -1, -1, -1, -1, -1}, // descriptor 1: tile 1 layer 1 has no property column
        {7, -1, 3, -1, -1, -1, -1, -1},   // descriptor 2: tile 0 layer 0
        {-1, 5, -1, -1, 9, -1, -1, -1},   // descriptor 3: tile 1 layer 0
    };
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 8; ++k) CHECK(out[(size_t)(8 * c + k)] == want[c][k]);
    // the same from records in another order (not sorted by tile and layer): first in the given order
    std::vector<covt_prop_info> shuffled = {pinfo[6], pinfo[3], pinfo[4], pinfo[0], pinfo[1]};
    std::fill(out.begin(), out.end(), 77);
    CHECK(where_bind(&w, ginfo.data(), 4, shuffled.data(), 5, (const uint8_t*)bytes, nb, out.data()) == COVT_OK);
    CHECK(out[16] == 1 && out[17] == -1 && out[18] == 3 && out[1] == 0 && out[25] == 5);
    // with fewer bytes the names at the end leave them
    std::fill(out.begin(), out.end(), 77);
    CHECK(where_bind(&w, ginfo.data(), 4, pinfo.data(), (int64_t)pinfo.size(), (const uint8_t*)bytes, 16, out.data()) == COVT_OK);
    CHECK(out[1] == -1 && out[25] == -1 && out[16] == 7 && out[18] == 3);
    // arguments
    CHECK(where_bind(nullptr, ginfo.data(), 4, pinfo.data(), 10, (const uint8_t*)bytes, nb, out.data()) == COVT_ERR_INVALID_ARG);
    CHECK(where_bind(&w, nullptr, 4, pinfo.data(), 10, (const uint8_t*)bytes, nb, out.data()) == COVT_ERR_INVALID_ARG);
    CHECK(where_bind(&w, ginfo.data(), 4, nullptr, 10, (const uint8_t*)bytes, nb, out.data()) == COVT_ERR_INVALID_ARG);
    CHECK(where_bind(&w, ginfo.data(), 4, pinfo.data(), 10, nullptr, nb, out.data()) == COVT_ERR_INVALID_ARG);
    CHECK(where_bind(&w, ginfo.data(), 4, pinfo.data(), 10, (const uint8_t*)bytes, nb, nullptr) == COVT_ERR_INVALID_ARG);
    CHECK(where_bind(&w, ginfo.data(), 0, pinfo.data(), 0, nullptr, 0, nullptr) == COVT_OK);
    ginfo[1].desc_index = 4;
    CHECK(where_bind(&w, ginfo.data(), 4, pinfo.data(), 10, (const uint8_t*)bytes, nb, out.data()) == COVT_ERR_INVALID_ARG);
    covt_where bad = w;
    bad.n_values = 33;
    ginfo[1].desc_index = 0;
    CHECK(where_bind(&bad, ginfo.data(), 4, pinfo.data(), 10, (const uint8_t*)bytes, nb, out.data()) == COVT_ERR_INVALID_ARG);
}

int main() {
    check_validation();
    check_compare();
    check_bind();
    printf("ok %ld\n", g_checks);
    return 0;
}

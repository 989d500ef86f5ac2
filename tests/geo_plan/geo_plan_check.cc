// geo_plan_check.cc -- TEST INFRASTRUCTURE: cov-tiles_amd/csrc/covt_geo_plan.h in a host-only program (no
// hipcc, no HIP runtime), built by tests/test_geo_ref.py with AddressSanitizer and UndefinedBehaviorSanitizer.
//
// Reads cases from stdin, one per line: <crs> <z> <x> <y> <extent> <px> <py>, and prints per case
//   <status> <sx> <ox> <sy> <oy as the bits of their doubles, hex> <kind> <X> <Y bits of the transformed pixel>
// (X, Y are the pixel itself for IDENTITY), so the test holds them against tests/covt_geo.py bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "covt_geo_plan.h"

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int main() {
    long long crs, z, x, y, e, px, py;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld", &crs, &z, &x, &y, &e, &px, &py) == 7) {
        covt_geo_xform t;
        const int st = geo_transform((int32_t)crs, (int32_t)z, (int32_t)x, (int32_t)y, (int32_t)e, t);
        double X = (double)(int32_t)px, Y = (double)(int32_t)py;
        if (st == COVT_OK && t.kind != COVT_GEO_IDENTITY) {
            X = geo_x(t, X);
            Y = t.kind == COVT_GEO_AFFINE_LAT ? geo_y<true>(t, Y) : geo_y<false>(t, Y);
        }
        // (the identity written as an affine map gives the pixel back bit for bit)
        const covt_geo_xform id = geo_identity_affine();
        if (bits(geo_x(id, (double)(int32_t)px)) != bits((double)(int32_t)px) ||
            bits(geo_y<false>(id, (double)(int32_t)py)) != bits((double)(int32_t)py))
            return 3;
        std::printf("%d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 "\n", st,
                    bits(t.sx), bits(t.ox), bits(t.sy), bits(t.oy), (int)t.kind, bits(X), bits(Y));
    }
    return 0;
}
